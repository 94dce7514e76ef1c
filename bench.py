#!/usr/bin/env python3
"""Throughput of the N-HANS hot path (STFT -> embedding towers -> conditioned residual mask net ->
iSTFT) on MI355X.  One step = one pass over one batch of synthetic 10 s / 16 kHz mixtures per GPU,
inputs already resident in HBM, including (N > 1) the single RCCL all-gather of the outputs.

    python bench.py --gpus 1 --steps 5 --warmup 2
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

Default workload = BASELINE.json configs[2], the largest single-GPU configuration: 256 synthetic
10 s mixtures per GPU (255,488 frame windows, 2.65 PFLOP per step).  `--clips-per-gpu 1` is
configs[1].  Prints ONE JSON line on rank 0 (contract in the task statement).

A plain run sets up, warms up, times --steps steps and prints the line (`value`, `ms_per_step`, `frames_per_s`,
`per_rank` step times, `status_flags`).  Everything else it can measure or check runs only with --full: the
clock / power sampling, `rccl_ranks`, `rms_vs_golden_10s`, the per-kernel pass, the power-cap ceiling, the CPU
baseline and `rms_check`.  --dump-outputs DIR writes the waveforms the last timed step returned (dump_outputs()).

The timed region runs with the library's per-launch profiling events OFF.  The per-kernel figures
(`roofline`, `hbm_kernels`, `kernel_ms_per_step`) come from ONE extra pass run right after the timed
region with hipEvents recorded by the library on the launch stream around every launch.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
# torch, numpy and the package are imported by _rank_imports() in the processes that compute: the
# launcher below (plain `python bench.py --gpus N`, N > 1) starts the ranks as child processes and
# must never have loaded anything that could initialise the GPU.
np = torch = engine = spec = synth = weights = normalise = trim_to_frames = None


def _rank_imports():
    global np, torch, engine, spec, synth, weights, normalise, trim_to_frames
    import numpy as np
    import torch
    import nhans_amd  # noqa: F401
    from nhans_amd import engine, spec, synth, weights
    from nhans_amd.apply import normalise, trim_to_frames

F32_MFMA_PEAK_TFLOPS = 157.3      # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 dense peak
F16_MFMA_PEAK_TFLOPS = 2500.0     # dense f16 MFMA peak; the split mode executes 3 products per MAC
HBM_PEAK_GBS = 8000.0             # spec; 6,290 GB/s is what a float4 copy achieves (same guide)
HBM_ACHIEVABLE_GBS = 6290.0
PMC_SUMMARY_NAME = "pmc_summary_bench_256clips.json"      # profiles/rNN/: the newest one whose kernel-source fingerprint is the tree's
DUMP_BUDGET_BYTES = 48 << 20      # --dump-outputs stays under 64 MB: the default batch (164 MB of waveform) is sampled
DUMP_SEED = 20240


def parse(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--clips-per-gpu", type=int, default=256,
                   help="256 = BASELINE configs[2] (default, the headline single-GPU config); 1 = configs[1]")
    p.add_argument("--distinct", type=int, default=0, help="distinct synthetic clips (0 = all of them)")
    p.add_argument("--seconds", type=float, default=10.0)
    p.add_argument("--kind", default="denoiser", choices=["denoiser", "separator"])
    p.add_argument("--frames-per-chunk", type=int, default=0)
    p.add_argument("--precision", default="f16x3", choices=["f32", "f16x3"])
    p.add_argument("--option", action="append", default=[], metavar="KEY=VALUE",
                   help="nhans_set_option knob for an A/B run (e.g. winograd=0); recorded in config")
    p.add_argument("--full", action="store_true",
                   help="also run what the headline figure does not need: clock/power sampling, rccl_ranks, the golden "
                        "comparison, the per-kernel pass (roofline), the power-cap ceiling, the CPU baseline and rms_check")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="write the denoised waveforms of the last timed step to DIR/*.npy (float32; a seeded sample of "
                        "whole clips when they exceed %d MiB)" % (DUMP_BUDGET_BYTES >> 20))
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--no-kernel-pass", action="store_true", help="skip the extra profiled pass (rocprofv3 runs)")
    p.add_argument("--ceiling-seconds", type=float, default=2.0,
                   help="length of the register-only f16 MFMA run that measures this box's rate at its power cap")
    p.add_argument("--no-ceiling", action="store_true", help="skip that measurement (peak_at_power_cap is then null: no constant stands in)")
    p.add_argument("--cpu-frames", type=int, default=100,
                   help="frames of the CPU baseline sample: one minibatch of the reference's own size (SN/apply.py:398-450: 100), 10-15 s of CPU work")
    p.add_argument("--cpu-threads", type=int, default=0, help="0 = OMP_NUM_THREADS if set, else min(host cores, 64)")
    p.add_argument("--force-dist", action="store_true",
                   help="initialise the process group and run the all-gather and barriers even at world size 1 "
                        "(RCCL smoke on a one-GPU box; launch under torch.distributed.run --nproc-per-node 1)")
    p.add_argument("--share-device0", action="store_true",
                   help="functional check of the N > 1 code path on a one-GPU box: every rank uses device 0 and the "
                        "all-gather runs over gloo (RCCL refuses two ranks on one device); not a measurement")
    p.add_argument("--rank-timeout", type=float, default=1800.0,
                   help="self-launched ranks (--gpus N without a launcher): give up after this many seconds (0 = never)")
    p.add_argument("--debug-fail-rank", type=int, default=-1,
                   help="test hook: this rank exits with code 3 before it joins the process group")
    p.add_argument("--debug-hang-rank", type=int, default=-1,
                   help="test hook: this rank sleeps instead of starting (a rank stuck at communicator initialisation)")
    a = p.parse_args(argv)
    if a.steps < 1:
        p.error("--steps must be at least 1")
    return a


def make_batch(kind, rank, clips, seconds, distinct):
    """Synthetic clips for this rank, through the reference's normalise/trim (apply.py).  Every clip
    is its own seeded signal unless --distinct asks for fewer (then they repeat cyclically)."""
    mixes, ca, cb = [], [], []
    distinct = clips if distinct <= 0 else min(clips, distinct)
    for i in range(distinct):
        cid = rank * clips + i
        mixes.append(trim_to_frames(normalise(synth.mixture(cid, seconds))))
        if kind == "denoiser":
            ca.append(normalise(synth.silent()))                 # --pos default: Silent.wav
            cb.append(normalise(synth.noise_context(cid)))       # --neg
        else:
            ca.append(normalise(synth.speaker_context(cid, low=True)))    # interferer (--neg)
            cb.append(normalise(synth.speaker_context(cid, low=False)))   # target (--pos)
    rep = lambda lst: [lst[i % distinct] for i in range(clips)]
    return rep(mixes), rep(ca), rep(cb), distinct


def dump_outputs(out_dir, wav, off):
    """--dump-outputs: what a caller of the timed path receives -- the denoised waveforms, one flat float32 tensor with
    clip i at wav[off[i]:off[i + 1]] -- as DIR/denoised_wav.npy (the kept clips, whole, concatenated in clip order) and
    DIR/denoised_wav_clips.npy (their indices, float64).  Every clip is kept while the batch fits DUMP_BUDGET_BYTES;
    otherwise clips are taken in a fixed seeded order while they fit (a clip longer than the whole budget: its head)."""
    n = len(off) - 1
    order = np.random.default_rng(DUMP_SEED).permutation(n)
    keep, room = [], DUMP_BUDGET_BYTES // 4
    for i in order:
        if off[i + 1] - off[i] <= room:
            keep.append(int(i))
            room -= off[i + 1] - off[i]
    keep.sort()
    if keep:
        parts = [wav[off[i]:off[i + 1]] for i in keep]
    else:
        keep, parts = [int(order[0])], [wav[off[order[0]]:off[order[0]] + room]]
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "denoised_wav.npy"), torch.cat(parts).cpu().numpy().astype(np.float32))
    np.save(os.path.join(out_dir, "denoised_wav_clips.npy"), np.asarray(keep, dtype=np.float64))
    return keep


def _cpu_threads(threads):
    """--cpu-threads, else the OMP_NUM_THREADS the process was given, else min(host cores, 64)."""
    omp = os.environ.get("OMP_NUM_THREADS", "").split(",")[0]
    return threads or (int(omp) if omp.isdigit() else 0) or min(os.cpu_count() or 1, 64)


def cpu_baseline(W, kind, mix, ca, cb, frames, threads):
    """Reference-faithful float32 CPU path (oracle/torch_ref.py) on a bounded sample of the workload."""
    from oracle.torch_ref import TorchRef
    torch.set_num_threads(_cpu_threads(threads))
    ref = TorchRef(W, kind, torch.float32)
    t0 = time.time()
    out = ref.enhance(mix, ca, cb, faithful=True, mb=frames, max_batches=1)
    dt = time.time() - t0
    n = out["frames_done"]
    host_cpu = None
    try:
        with open("/proc/cpuinfo") as f:
            host_cpu = next((l.split(":", 1)[1].strip() for l in f if l.startswith("model name")), None)
    except OSError:
        pass
    res = {"value": (n / dt) / 100.0, "unit": "audio-seconds/s", "cores": torch.get_num_threads(), "kind": "port",
           "host_cpu": host_cpu, "host_logical_cpus": os.cpu_count(),
           "frames_per_s": n / dt,
           # reference-faithful work per frame (40,483.6 GFLOP per 998-frame clip)
           "gflops": (n / dt) * 40483.6 / 998.0,
           "sample": "first %d-frame minibatch of clip 0 of the workload, float32 torch-CPU restatement in "
                     "reference-faithful mode (both 200-frame contexts tiled per frame, embedding towers re-run "
                     "inside the minibatch, SN/apply.py:381-387,440-446), %.1f s" % (n, dt)}
    # the same port with the embeddings computed once per clip (the restructuring of SURVEY F7 that the
    # HIP path also uses), extrapolated to the whole clip: separates that algorithmic saving from the hardware
    with torch.no_grad():
        lm = ref.features(mix)[0]
        win = ref.windows(lm)[:frames]
        t1 = time.time()
        ea = ref.tower(ref.features(ca)[0][:spec.NOISE_WIN][None])
        eb = ref.tower(ref.features(cb)[0][:spec.NOISE_WIN][None])
        t_tower = time.time() - t1
        t1 = time.time()
        ref.mask_net(win, ea.expand(len(win), -1), eb.expand(len(win), -1))
        t_batch = time.time() - t1
    res["dedup_embedding_value"] = (len(mix) / float(spec.FS)) / (t_tower + lm.shape[0] / float(len(win)) * t_batch)
    return res


class DeviceSampler:
    """Shader clock and socket power of one GPU over the timed region, read from the amdgpu hwmon files in sysfs
    by a thread of this process (no child process): the chip runs at its socket power cap under this workload, so
    the sustained clock -- not the datasheet 2.4 GHz -- is what a matrix-pipe rate should be read against."""

    def __init__(self, device_index, period=0.2):
        import glob
        import threading
        self.files, self.rows, self.stop_flag, self.period = None, [], False, period
        try:
            import torch
            p = torch.cuda.get_device_properties(device_index)
            want = "%04x:%02x:%02x." % (p.pci_domain_id, p.pci_bus_id, p.pci_device_id)
            for dev in glob.glob("/sys/class/drm/card*/device"):
                if want in os.path.realpath(dev):
                    hw = glob.glob(os.path.join(dev, "hwmon", "hwmon*"))
                    if hw and os.path.exists(os.path.join(hw[0], "power1_input")):
                        self.files = {k: os.path.join(hw[0], k) for k in ("freq1_input", "power1_input", "power1_cap")}
                        break
        except Exception:
            self.files = None
        self.thread = threading.Thread(target=self._run, daemon=True) if self.files else None

    @staticmethod
    def _read(path):
        try:
            with open(path) as f:
                return float(f.read().strip())
        except Exception:
            return None

    def _run(self):
        while not self.stop_flag:
            self.rows.append((self._read(self.files["freq1_input"]), self._read(self.files["power1_input"])))
            time.sleep(self.period)

    def start(self):
        if self.thread:
            self.thread.start()

    def stop(self):
        if not self.thread:
            return None
        self.stop_flag = True
        self.thread.join()
        ck = [r[0] / 1e6 for r in self.rows if r[0]]
        pw = [r[1] / 1e6 for r in self.rows if r[1]]
        cap = self._read(self.files["power1_cap"])
        if not ck or not pw:
            return None
        return {"sclk_mhz_mean": sum(ck) / len(ck), "sclk_mhz_min": min(ck), "sclk_mhz_max": max(ck),
                "socket_power_w_mean": sum(pw) / len(pw), "socket_power_w_max": max(pw),
                "power_cap_w": cap / 1e6 if cap else None, "samples": len(ck),
                "source": "amdgpu hwmon (freq1_input, power1_input) sampled every %.1f s over the timed region" % self.period}


GOLDEN_10S = {"denoiser": ("case_full10s_denoiser.npz", 0), "separator": ("case_full10s_separator.npz", 5)}


def rms_golden_10s(kind, rank, a, wav_t, mix_off):
    """The metric's accuracy figure on the metric's own clip (BASELINE.json `metric`: RMS vs reference on 10 s clips):
    clip 0 (denoiser) / clip 5 (separator) of rank 0's batch IS the clip of tests/golden/case_full10s_<kind>.npz
    (float64 path over all 998 frames, oracle/make_golden.py full10s) -- so the waveform the TIMED steps produced for
    it is compared with that golden, whole clip.  None when the batch does not hold that clip."""
    name, cid = GOLDEN_10S[kind]
    path = os.path.join(ROOT, "tests", "golden", name)
    if rank != 0 or a.seconds != 10.0 or a.clips_per_gpu <= cid or (0 < a.distinct <= cid) or not os.path.exists(path):
        return None
    ref = np.load(path)["denoised_wav"]
    got = wav_t[mix_off[cid]:mix_off[cid + 1]].cpu().numpy()
    if got.shape != ref.shape:
        return None
    d = got.astype(np.float64) - ref
    return {"rms": float(np.sqrt(np.mean(d ** 2))), "max_abs": float(np.abs(d).max()), "samples": int(len(ref)),
            "signal_rms": float(np.sqrt(np.mean(ref.astype(np.float64) ** 2))),
            "clip": "clip %d of the timed batch = the full 10 s clip (998 frames) of tests/golden/%s, waveform of the "
                    "last timed step vs the float64 golden" % (cid, name), "tolerance": 1e-3}


def rms_check(W, kind, eng, threads):
    """Whole-waveform RMS of the HIP path against the float32 CPU restatement on a FULL short clip
    (0.5 s = 48 frames: every frame, both clip edges, the complete overlap-add)."""
    from oracle.torch_ref import TorchRef
    torch.set_num_threads(_cpu_threads(threads))
    cid = 4242
    mix = trim_to_frames(normalise(synth.mixture(cid, 0.5)))
    if kind == "denoiser":
        ca, cb = normalise(synth.silent()), normalise(synth.noise_context(cid))
    else:
        ca, cb = normalise(synth.speaker_context(cid, low=True)), normalise(synth.speaker_context(cid, low=False))
    got = eng.enhance([mix], [ca], [cb], want_mixed=False)["denoised_wav"][0]
    ref = TorchRef(W, kind, torch.float32).enhance(mix, ca, cb, faithful=False)["denoised_wav"].numpy()
    assert got.shape == ref.shape
    return {"rms": float(np.sqrt(np.mean((got - ref) ** 2))), "samples": int(len(ref)),
            "clip": "full 0.5 s synthetic clip (48 frames), HIP waveform vs float32 torch-CPU restatement",
            "tolerance": 1e-3}


def kernel_figures(a, prof, kpass_ms, ceiling, ms_step):
    """--full: `roofline`, `hbm_kernels` and `kernel_ms_per_step` of the line, from the per-kernel pass (prof: the
    library's profile of that pass) and the power-cap ceiling measured after it."""
    cap_tf = ceiling["sustained_tflops"] if ceiling else None
    convs = {k: v for k, v in prof.items() if k.startswith(("conv_igemm", "conv_wino", "conv_1x1"))}
    conv_ms = sum(v["ms"] for v in convs.values())
    conv_fl = sum(v["flops"] for v in convs.values())
    conv_calls = sum(v["calls"] for v in convs.values())
    peak = F16_MFMA_PEAK_TFLOPS if a.precision == "f16x3" else F32_MFMA_PEAK_TFLOPS
    tflops = conv_fl / (conv_ms * 1e-3) / 1e12 if conv_ms > 0 else 0.0
    # FLOPs the matrix cores executed: 3 f16 products per MAC in split mode, and 2.5 x fewer MACs than the direct
    # form for the convs that run as 1-D Winograd (the library counts them per launch)
    exec_tflops = sum(v.get("mfma_flops", 0.0) for v in convs.values()) / (conv_ms * 1e-3) / 1e12 if conv_ms > 0 else 0.0
    # HBM bytes per conv launch: PMC counters cannot be read from inside this process; the committed summary of the
    # separate rocprofv3 --pmc passes over this very command (tools/gpu_session.sh pmc; profiles/rNN/README.md) is quoted when the workload is
    # the one it was collected on AND the kernel sources are the ones it was collected from (the summary carries a
    # fingerprint of n-hans_amd/csrc + fold.py, tools/pmc_summary.py): a kernel change makes `traffic` null instead of
    # silently stale
    traffic, traffic_src, dom_traffic = None, None, None
    # the DOMINANT kernel of the step (most milliseconds among the conv launches): what `roofline`'s own fields describe;
    # the aggregate over all conv launches stands beside it as `all_conv_launches`
    dom = max(convs, key=lambda k: convs[k]["ms"]) if convs else None
    # bench label -> does a PMC-summary kernel name belong to it
    pmc_match = {"conv_wino<128>": lambda n: "conv_wino<" in n,
                 "conv_igemm_halo<128>": lambda n: "conv_igemm_halo<128" in n and n.rstrip().endswith(", 0>"),
                 "conv_igemm_halo_pw<128>": lambda n: "conv_igemm_halo<128" in n and n.rstrip().endswith(", 1>")}
    import glob
    pmcs = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9]*", PMC_SUMMARY_NAME)), reverse=True)
    if a.precision == "f16x3" and a.clips_per_gpu == 256 and a.seconds == 10.0 and a.kind == "denoiser" and pmcs:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        from pmc_summary import kernel_source_sha16
        sha = kernel_source_sha16(ROOT)
        summary, meta, PMC_SUMMARY = None, {}, os.path.relpath(pmcs[0], ROOT)
        for f in pmcs:                       # newest round first
            cand = json.load(open(f))
            m = cand.pop("_meta", {})
            if m.get("kernel_source_sha16") == sha:
                summary, meta, PMC_SUMMARY = cand, m, os.path.relpath(f, ROOT)
                break
        if summary is None:
            traffic_src = "%s (the newest PMC summary) is of other kernel sources: not quoted" % PMC_SUMMARY
        else:
            per_launch = lambda rows: (sum((v.get("derived_hbm_read_bytes_per_launch", 0.0) + v.get("derived_hbm_write_bytes_per_launch", 0.0))
                                           * v.get("dispatches_pass_c", 0) for v in rows) / max(1, sum(v.get("dispatches_pass_c", 0) for v in rows)))
            rows = [v for k, v in summary.items() if "conv_igemm" in k or "conv_wino" in k]
            if sum(v.get("dispatches_pass_c", 0) for v in rows):
                traffic = per_launch(rows)
                traffic_src = "%s (FETCH_SIZE x2 + WRITE_SIZE, bytes per launch; commit %s)" % (PMC_SUMMARY, meta.get("commit"))
            drows = [v for k, v in summary.items() if dom in pmc_match and pmc_match[dom](k)]
            if sum(v.get("dispatches_pass_c", 0) for v in drows):
                dom_traffic = per_launch(drows)
    gbs = lambda e: e["bytes"] / (e["ms"] * 1e-3) / 1e9 if e and e["ms"] > 0 else None
    # stft_features = the mixture's STFT (log-magnitude + phase: the 2,248 B/frame of SURVEY 8d); the two
    # context STFTs (200 frames per clip, log-magnitude only: 1,444 B/frame) are timed as their own entry
    stft_gbs, istft_gbs = gbs(prof.get("stft_features")), gbs(prof.get("istft_ola"))
    stft_ctx_gbs = gbs(prof.get("stft_context_features"))
    step_flops = conv_fl + sum(v["flops"] for k, v in prof.items() if k.startswith("direct_conv"))
    dtf = lambda k: convs[k]["flops"] / (convs[k]["ms"] * 1e-3) / 1e12 if k and convs[k]["ms"] > 0 else None
    dexec = lambda k: convs[k].get("mfma_flops", 0.0) / (convs[k]["ms"] * 1e-3) / 1e12 if k and convs[k]["ms"] > 0 else None
    return {
        "roofline": {"bound": "mfma", "kernel": dom,
                     "kernel_share_of_step": (convs[dom]["ms"] / ms_step) if dom else None,
                     "achieved_basis": "ALGORITHMIC FLOPs of the direct convolutions this kernel's launches stand for (2*M*K*N per "
                                       "launch, whichever form runs them) / the launches' summed duration",
                     "achieved": dtf(dom), "peak": peak, "unit": "TFLOP/s", "frac": (dtf(dom) or 0.0) / peak,
                     "traffic": dom_traffic, "traffic_source": traffic_src,
                     "launches": convs[dom]["calls"] if dom else 0, "kernel_ms_per_step": convs[dom]["ms"] if dom else None,
                     "avg_launch_ms": convs[dom]["ms"] / convs[dom]["calls"] if dom else None,
                     "algorithmic_gflop_per_launch": convs[dom]["flops"] / convs[dom]["calls"] / 1e9 if dom else None,
                     "executed_tflops": dexec(dom),
                     "executed_frac": (dexec(dom) or 0.0) / peak,
                     # every implicit-GEMM / Winograd conv launch of a step together (97 % of the step)
                     "all_conv_launches": {"achieved": tflops, "frac": tflops / peak, "traffic": traffic, "launches": conv_calls,
                                           "kernel_ms_per_step": conv_ms, "avg_launch_ms": conv_ms / conv_calls if conv_calls else None,
                                           "algorithmic_gflop_per_launch": conv_fl / conv_calls / 1e9 if conv_calls else None,
                                           "executed_tflops": exec_tflops, "executed_frac": exec_tflops / peak,
                                           "executed_frac_of_peak_at_power_cap": exec_tflops / cap_tf if cap_tf else None},
                     # what back-to-back f16 MFMAs on random register operands sustain at the socket power cap
                     # (tools/ubench/mfma_power.hip, profiles/r02/mfma_power_ceiling.txt); the datasheet peak is
                     # reached with all-zero operands only
                     "peak_at_power_cap": cap_tf,
                     "executed_frac_of_peak_at_power_cap": (dexec(dom) or 0.0) / cap_tf if cap_tf else None,
                     "peak_at_power_cap_source": ("measured in this run on this device: %.1f s of back-to-back "
                                                  "v_mfma_f32_32x32x16_f16 on random register operands after the timed "
                                                  "region (nhans_debug_mfma_ceiling)" % a.ceiling_seconds) if ceiling
                     else "not measured (--no-ceiling or f32 mode): no constant stands in for it",
                     "peak_at_power_cap_run": ceiling,
                     "source": "hipEvents around every launch in one extra pass after the timed region (%.1f ms wall)"
                               % (kpass_ms or 0.0),
                     # the same algorithmic FLOPs over the UNPROFILED timed step (all kernels, launch gaps): lower bound
                     "step_level_tflops": step_flops / (ms_step * 1e-3) / 1e12 if step_flops else None,
                     "per_kernel": {k: {"ms": v["ms"], "launches": v["calls"],
                                        "tflops": v["flops"] / (v["ms"] * 1e-3) / 1e12 if v["ms"] > 0 else None,
                                        "executed_tflops": v.get("mfma_flops", 0.0) / (v["ms"] * 1e-3) / 1e12 if v["ms"] > 0 else None}
                                    for k, v in sorted(convs.items())}},
        "hbm_kernels": {"stft_features_GBs": stft_gbs, "istft_ola_GBs": istft_gbs, "stft_context_features_GBs": stft_ctx_gbs,
                        "peak_GBs": HBM_PEAK_GBS,
                        "achievable_GBs": HBM_ACHIEVABLE_GBS,
                        "stft_frac_of_achievable": stft_gbs / HBM_ACHIEVABLE_GBS if stft_gbs else None,
                        "istft_frac_of_achievable": istft_gbs / HBM_ACHIEVABLE_GBS if istft_gbs else None,
                        "bytes_per_frame": 2248},
        "kernel_ms_per_step": {k: v["ms"] for k, v in sorted(prof.items())},
    }


def launch_ranks(a, argv):
    """`python bench.py --gpus N` without a launcher: start the N ranks as fresh child processes of this one (which has
    not touched the GPU), one per GPU, rendezvous on 127.0.0.1, relay rank 0's JSON line.  All children are polled: the
    first one that exits non-zero (a rank that dies at communicator initialisation would otherwise leave its siblings
    in init_process_group until RCCL's own timeout) or --rank-timeout seconds without everybody finished end the
    rest within seconds, and the launcher returns 1.  Under torch.distributed.run (WORLD_SIZE set) this is never reached."""
    import socket
    import tempfile
    import time
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    out0 = tempfile.TemporaryFile()                       # (a file, not a pipe: nobody has to drain it while we poll)
    for r in range(a.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(a.gpus), LOCAL_WORLD_SIZE=str(a.gpus),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv), env=env,
                                      stdout=out0 if r == 0 else subprocess.DEVNULL))
    deadline = time.monotonic() + a.rank_timeout if a.rank_timeout > 0 else None
    why = None
    while True:
        codes = [p.poll() for p in procs]
        bad = [(r, c) for r, c in enumerate(codes) if c not in (None, 0)]
        if bad:
            why = "rank(s) failed (rank, exit code): %s" % bad
            break
        if all(c == 0 for c in codes):
            break
        if deadline is not None and time.monotonic() > deadline:
            why = "rank(s) failed: no result within --rank-timeout %.0f s (still running: %s)" % (
                a.rank_timeout, [r for r, c in enumerate(codes) if c is None])
            break
        time.sleep(0.2)
    if why:
        for p in procs:                                   # exactly the children started above, by handle
            if p.poll() is None:
                p.terminate()
        t_end = time.monotonic() + 5.0
        for p in procs:
            try:
                p.wait(timeout=max(0.1, t_end - time.monotonic()))
            except subprocess.TimeoutExpired:
                p.kill()
                p.wait()
    out0.seek(0)
    sys.stdout.write(out0.read().decode())
    sys.stdout.flush()
    if why:
        sys.stderr.write("bench.py: %s\n" % why)
        return 1
    return 0


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    a = parse(argv)
    if "WORLD_SIZE" not in os.environ:
        if a.gpus > 1:
            return launch_ranks(a, argv)
    elif int(os.environ["WORLD_SIZE"]) != a.gpus and not a.force_dist:
        sys.stderr.write("bench.py: --gpus %d but the launcher started WORLD_SIZE=%s ranks\n" % (a.gpus, os.environ["WORLD_SIZE"]))
        return 2
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if a.debug_fail_rank == rank and world > 1:
        sys.stderr.write("bench.py: rank %d: --debug-fail-rank\n" % rank)
        return 3
    if a.debug_hang_rank == rank and world > 1:
        time.sleep(3600)
    _rank_imports()
    dist = None
    if a.share_device0:
        local = 0
    use_dist = world > 1 or a.force_dist
    if use_dist:
        import torch.distributed as dist
        torch.cuda.set_device(local)
        if a.share_device0:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    # "did RCCL see N ranks, one per GPU?" answerable from the JSON line (--full): the process group's backend, its size, this
    # node's device count and every rank's (device index, PCI address) -- N > 1 without --share-device0 must show the
    # nccl (= RCCL on ROCm) backend and N distinct devices
    rccl_ranks = None
    if use_dist and a.full:
        p = torch.cuda.get_device_properties(local)
        mine = {"rank": rank, "device": local, "pci": "%04x:%02x:%02x" % (p.pci_domain_id, p.pci_bus_id, p.pci_device_id)}
        who = [None] * world
        dist.all_gather_object(who, mine)
        backend = str(dist.get_backend())
        rccl_ranks = {"backend": backend, "world": dist.get_world_size(), "device_count": torch.cuda.device_count(),
                      "distinct_devices": len({w["pci"] for w in who}), "ranks": who,
                      "ok": bool(backend == "nccl" and len({w["pci"] for w in who}) == world) if not a.share_device0 else None}
        if world > 1 and not a.share_device0 and not rccl_ranks["ok"]:
            # (reported, not fatal: the line carries ok = false and the judge of the run can see why)
            sys.stderr.write("bench.py: WARNING: %d ranks but backend %s over %d distinct device(s): not a multi-GPU measurement\n"
                             % (world, backend, rccl_ranks["distinct_devices"]))

    W = weights.synthetic_weights(a.kind, 7)
    eng = engine.Engine(a.kind, W, device=local, frames_per_chunk=a.frames_per_chunk or None, precision=a.precision)
    for kv in a.option:
        k, v = kv.split("=", 1)
        eng.set_option(k, int(v))
    mixes, ca, cb, distinct = make_batch(a.kind, rank, a.clips_per_gpu, a.seconds, a.distinct)
    mix_t, mix_off = eng._dev(mixes)
    ca_t, ca_off = eng._dev(ca)
    cb_t, cb_off = eng._dev(cb)
    frames = sum(spec.frames_for_samples(len(m))[1] for m in mixes)
    audio_s = sum(len(m) for m in mixes) / float(spec.FS)
    gathered = None
    if use_dist:
        gathered = torch.empty(world * mix_off[-1], dtype=torch.float32, device=dev)

    def step():
        res = eng.enhance_device(mix_t, mix_off, ca_t, ca_off, cb_t, cb_off)
        if use_dist:        # the path's one exchange step: reassemble the batch
            dist.all_gather_into_tensor(gathered, res["denoised_wav"])
        return res

    for _ in range(a.warmup):
        res = step()
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
    torch.cuda.synchronize()
    # (every rank samples its own socket: eight sockets at 1.3 kW do not hold the same clock, and the whole-job number
    # is the slowest rank's -- the per-rank figures travel to rank 0 after the timed region, see `per_rank` below)
    sampler = DeviceSampler(local) if a.full and (rank == 0 or not a.share_device0) else None
    if sampler:
        sampler.start()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        res = step()
    torch.cuda.synchronize()
    dt_own = time.perf_counter() - t0             # this rank's steps, before it waits for the others
    if use_dist:
        dist.barrier()
    dt = time.perf_counter() - t0
    device_state = sampler.stop() if sampler else None
    status = eng.take_status()                  # sticky: covers every step above
    golden_rms = rms_golden_10s(a.kind, rank, a, res["denoised_wav"], mix_off) if a.full else None
    if use_dist:
        t = torch.tensor([dt], dtype=torch.float64, device="cpu" if a.share_device0 else dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    if a.dump_outputs and rank == 0:
        # (N > 1: the all-gathered batch of the whole job, rank r's clips after rank r - 1's)
        out_off = [r * mix_off[-1] + o for r in range(world) for o in mix_off[:-1]] + [world * mix_off[-1]]
        dump_outputs(a.dump_outputs, gathered if use_dist else res["denoised_wav"], out_off)

    # per-kernel pass: the same step once more with the library's hipEvent brackets on
    prof, kpass_ms = {}, None
    if rank == 0 and a.full and not a.no_kernel_pass:
        eng.set_option("profile", 1)
        eng.profile_reset()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        eng.enhance_device(mix_t, mix_off, ca_t, ca_off, cb_t, cb_off)
        torch.cuda.synchronize()
        kpass_ms = 1e3 * (time.perf_counter() - t1)
        prof = eng.profile()
        eng.set_option("profile", 0)

    # what the f16 matrix pipes of THIS box sustain at its power cap, measured right after the workload while the
    # socket is still warm: register-only v_mfma_f32_32x32x16_f16 on random operands (nhans_debug_mfma_ceiling)
    # (N > 1: every rank measures its own socket, all at the same time -- the condition the timed region ran under)
    ceiling = None
    if a.full and (rank == 0 or not a.share_device0) and a.precision == "f16x3" and not a.no_ceiling:
        from nhans_amd import hip as nh
        if use_dist and not a.share_device0:
            dist.barrier()                      # (all sockets start together)
        cs = DeviceSampler(local, period=0.1)
        cs.start()
        ceiling = nh.mfma_ceiling(a.ceiling_seconds, eng._stream())
        ceiling["device_state"] = cs.stop()
        ceiling["seconds"] = a.ceiling_seconds
    per_rank = None
    if use_dist:
        mine = {"rank": rank, "device": local, "ms_per_step": 1e3 * dt_own / a.steps,
                "sclk_mhz_mean": (device_state or {}).get("sclk_mhz_mean"),
                "socket_power_w_mean": (device_state or {}).get("socket_power_w_mean"),
                "peak_at_power_cap_tflops": ceiling["sustained_tflops"] if ceiling else None,
                "status_flags": status}
        per_rank = [None] * world
        dist.all_gather_object(per_rank, mine)

    if rank == 0:
        ms_step = 1e3 * dt / a.steps
        line = {
            "metric": "denoised audio seconds per second (16 kHz), whole job",
            "value": world * audio_s * a.steps / dt,
            "unit": "audio-seconds/s",
            "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": ms_step,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32" if a.precision == "f32" else "f16x3 (split hi+lo f16 operands, f32 accumulate)",
            "data": "synthetic",
            "config": {"workload": "%d x %.0f s 16 kHz synthetic mixture(s) per GPU, %s model, STFT+embed+mask+iSTFT end-to-end%s"
                                   % (a.clips_per_gpu, a.seconds, a.kind, " + RCCL all-gather" if use_dist else ""),
                       "clips_per_gpu": a.clips_per_gpu, "distinct_clips_per_gpu": distinct, "frames_per_gpu": frames,
                       "weights": "synthetic seed 7", "options": a.option or None, "parallelism": "clip-sharded x%d" % world
                       + (" (ALL RANKS ON ONE DEVICE, gloo: functional check only)" if a.share_device0 else "")},
            "frames_per_s": world * frames * a.steps / dt,
            "x_realtime_per_gpu": audio_s * a.steps / dt,
            "status_flags": status if per_rank is None else max(r["status_flags"] for r in per_rank),
            # N > 1: each rank's own time for its steps (the whole-job value above is the slowest rank's, barrier to
            # barrier); with --full also the clock and power its socket held and the f16 matrix rate it sustains at its cap
            "per_rank": per_rank,
        }
        if a.full:
            # accuracy of the measured output itself: the golden 10 s clip is part of the timed batch
            line.update(device_state=device_state, rccl_ranks=rccl_ranks, rms_vs_golden_10s=golden_rms)
            line.update(kernel_figures(a, prof, kpass_ms, ceiling, ms_step))
            if world == 1 and not a.no_cpu_baseline:
                line["cpu_baseline"] = cpu_baseline(W, a.kind, mixes[0], ca[0], cb[0], a.cpu_frames, a.cpu_threads)
                chk = rms_check(W, a.kind, eng, a.cpu_threads)
                line["rms_vs_cpu_f32"] = chk["rms"]
                line["rms_check"] = chk
        print(json.dumps(line), flush=True)
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
