"""Drop-in API surface of N-HANS inference on MI355X.

Mirrors the reference's entry points -- same names, argument meaning, file outputs and error
behaviour -- with the TensorFlow graph calls replaced by the HIP library (engine.Engine):

    apply_snc(mixedpath, pospath, negpath, save_to)        SN/apply.py:339-472
    apply_denoiser(mixedpath, negpath, save_to)            SN/apply.py:478-481
    apply_separator(mixedpath, cleanpath, noisepath, save_to)   SS/apply.py:288-397
    main() for the `nhans_denoiser` / `nhans_separator` console scripts   setup.py:44-50,
        flags --input --neg --pos --output --compensate --ac            SN/apply.py:29-35

Host code here is I/O only: wav reading/normalising/trimming (numpy, float64 like the reference),
writing float32 wavs, and the denoiser's removed/compensated side outputs.

Deviations that the tree forces (documented in DESIGN.md):
  * Conditioning recordings shorter than 200 frames (32,240 samples) crash the in-tree reference
    (`tf.reshape(..., [200, 201])`, SN/apply.py:381-382) although its own examples are 1 s long.
    They are repeated to the needed length with the reference's own repeat rule for short noise
    (`domixing`, SN/apply.py:60-66).
  * `./audio_examples/Silent.wav` (default --pos) is all zeros; if the file is absent an all-zero
    recording is used.
  * Weights: `./trained_model/<bundle>` relative to the CWD as in the reference (or
    $NHANS_MODEL_DIR).  The bundles in the reference tree are git-LFS pointers; loading one raises
    unless synthetic weights are requested explicitly (--weights synthetic / NHANS_WEIGHTS=synthetic).
"""
import argparse
import os
import sys

import numpy as np
from scipy.io.wavfile import read as wavread
from scipy.io.wavfile import write as wavwrite

from . import spec

Fs = spec.FS
Noise_Win = spec.NOISE_WIN
Mix_Win = spec.MIX_WIN

DENOISER_BUNDLE = "81448_0-1000000"      # SN/apply.py:431-432
SEPARATOR_BUNDLE = "81457_2-545000"      # SS/apply.py:371-372

_engines = {}
_lite = {}               # torch-free engines of the single-process command line (lite.py)
_device_index = 0
TIMING = None            # --timing: dict of the seconds each start-up step took (printed as JSON on stderr)


class Flags(object):
    """Stand-in for the reference's absl FLAGS (SN/apply.py:29-35)."""
    input = "./audio_examples/mixed.wav"
    neg = "./audio_examples/game_noise.wav"
    pos = "./audio_examples/Silent.wav"
    output = "./audio_examples/denoised.wav"
    compensate = 0.0
    ac = False
    convert = False      # library calls keep the in-tree asserts; the CLI converts like the packaged tool
    Fs = Fs
    weights = os.environ.get("NHANS_WEIGHTS", "checkpoint")
    model_dir = os.environ.get("NHANS_MODEL_DIR", "./trained_model")
    cache = True         # folded-blob cache (blobcache.py); --no-cache folds the weights in this process
    online_ms = None     # --online_ms: file mode through the online path (online.py) in pieces of this many ms
    convert_on = "host"  # --convert_on gpu: format / rate conversion and normalisation of the files on the device (resample.py)
    output_rate = "16000"    # --output_rate input: the output files at the input file's rate (converted back on the device)
    highband = None      # --highband G: the input's own band above 8 kHz, times G, added to the files written at the input's rate (live.fullband_mix)
    score_against = None # --score_against TARGET: score the files written against a clean target on the device (score.py)
    score_out = None     # --score_out PATH.json: where the scores go (stdout otherwise)
    bss = False          # --bss: with --score_against and --interferer, also SDR, SIR and SAR (score.py: bss_reference is the definition)
    interferer = None    # --interferer FILE: the signal that was to be removed, for --bss
    align_ms = None      # --align_ms MS: with --score_against, the delay of the denoised file against the target is estimated within MS and taken out
    align_drift = False  # --align_drift: with --align_ms, a line is fitted to the delay over the file and warped out (Context.align_drift)
    quality = False      # --quality: with --score_against, also LLR, cepstral distance and fwSegSNR (score.py: quality_reference is the definition)
    stoi = False         # --stoi: with --score_against, also STOI and extended STOI (score.py: stoi_reference is the definition)
    phase_iters = 0      # --phase_iters N: Griffin-Lim iterations on the denoised rows before their iSTFT (include/nhans_hip.h: "phase_iters")
    phase_alpha = 0.0    # --phase_alpha A: their momentum, 0 <= A < 1
    array = None         # --array mvdr: a multi-channel input keeps its channels and goes through Context.enhance_array (mask-driven MVDR)
    array_ref = 0        # --array_ref R: the reference channel
    array_post = "none"  # --array_post none|mask|net: what follows the beamformer
    lookahead_ms = 10 * spec.LOOKAHEAD   # --lookahead_ms: 10 ms per frame of look-ahead (include/nhans_hip.h: "lookahead"), 170 = all 17


FLAGS = Flags()


# ------------------------------------------------------------------------------ wav front end
def read_wav(in_path):
    """Contract of the reference's reader (SN/apply.py:46-53): 16 kHz int16 PCM only, anything else
    is an AssertionError; a multi-channel file comes back as the float64 mean of its channels."""
    rate, pcm = wavread(in_path)
    if rate != FLAGS.Fs:
        raise AssertionError("%s: sample rate %d Hz, expected %d" % (in_path, rate, FLAGS.Fs))
    if pcm.dtype != np.int16:
        raise AssertionError("%s: sample format %s, expected int16" % (in_path, pcm.dtype))
    return pcm if pcm.ndim == 1 else pcm.mean(axis=1)


def read_wav_any(in_path):
    """Format converter of the packaged tool (README.md:42: other formats are "automatically
    converted" to 16 kHz / 16-bit PCM with sox; sox is not available, scipy does the same job):
    any PCM/float wav at any rate -> what read_wav() would have returned for the converted file."""
    rate, samples = wavread(in_path)
    if rate == FLAGS.Fs and samples.dtype == np.int16:        # already what read_wav() accepts
        return samples if samples.ndim == 1 else samples.mean(axis=1)
    x = samples.astype(np.float64)
    if samples.dtype == np.uint8:
        x = (x - 128.0) * 256.0
    elif samples.dtype == np.int32:
        x = x / 65536.0
    elif samples.dtype.kind == 'f':
        x = x * 32768.0
    if rate != FLAGS.Fs:
        from math import gcd
        from scipy.signal import resample_poly
        g = gcd(int(FLAGS.Fs), int(rate))
        x = resample_poly(x, FLAGS.Fs // g, rate // g, axis=0)
    x = np.clip(np.round(x), -32768, 32767).astype(np.int16)
    if x.ndim > 1:
        x = x.mean(axis=1)
    return x


def _reader():
    return read_wav_any if getattr(FLAGS, 'convert', False) else read_wav


def read_wav_channels(in_path):
    """--array: the input with its channels kept, int16-scale values [n, C] -- read_wav's contract, or with the converter
    read_wav_any's steps, each without the mean over the channels."""
    rate, samples = wavread(in_path)
    if samples.ndim != 2 or samples.shape[1] < 2:
        raise ValueError("%s: --array needs more than one channel" % in_path)
    if not getattr(FLAGS, 'convert', False):
        if rate != FLAGS.Fs:
            raise AssertionError("%s: sample rate %d Hz, expected %d" % (in_path, rate, FLAGS.Fs))
        if samples.dtype != np.int16:
            raise AssertionError("%s: sample format %s, expected int16" % (in_path, samples.dtype))
        return samples
    if rate == FLAGS.Fs and samples.dtype == np.int16:
        return samples
    x = samples.astype(np.float64)
    if samples.dtype == np.uint8:
        x = (x - 128.0) * 256.0
    elif samples.dtype == np.int32:
        x = x / 65536.0
    elif samples.dtype.kind == 'f':
        x = x * 32768.0
    if rate != FLAGS.Fs:
        from math import gcd
        from scipy.signal import resample_poly
        g = gcd(int(FLAGS.Fs), int(rate))
        x = resample_poly(x, FLAGS.Fs // g, rate // g, axis=0)
    return np.clip(np.round(x), -32768, 32767).astype(np.int16)


def handle_array_signals(mixedpath, a_path, b_path):
    """--array: (ctx_a, ctx_b, mixed [n, C]) float32.  Every channel is divided by what the file is divided by today, the
    peak of the channels' mean + 1e-6, so that the mean of the channels is today's signal; trimmed to whole frames."""
    try:
        x = read_wav_channels(mixedpath)
        peak = np.max(np.abs(x.mean(axis=1))) if len(x) else 0
        mixed = (x / (peak + 0.000001)).astype(np.float32)
        spare = (len(mixed) - spec.WIN) % spec.HOP
        mixed = mixed[:len(mixed) - spare] if spare else mixed
        if len(mixed) < spec.WIN:
            raise ValueError("%s: shorter than one %d-sample STFT window" % (mixedpath, spec.WIN))
        return normalise(_read_context(a_path)), normalise(_read_context(b_path)), mixed
    except Exception:
        print('error in threads')
        print(mixedpath, a_path, b_path)
        return None


def _array_kw():
    return {"ref": int(FLAGS.array_ref), "post": FLAGS.array_post, "mask_from": "mean", "want_mixed": True}


def _enhance_arrays(eng, mixes, ca, cb):
    """--array: [(denoised, mixed_processed)] per clip; the clips of one channel count go through one enhance_array call."""
    outs = [None] * len(mixes)
    for C in sorted({m.shape[1] for m in mixes}):
        idx = [i for i, m in enumerate(mixes) if m.shape[1] == C]
        if not 0 <= int(FLAGS.array_ref) < C:
            raise ValueError("--array_ref %d: the input has %d channels" % (FLAGS.array_ref, C))
        res = eng.enhance_array([mixes[i] for i in idx], [ca[i] for i in idx], [cb[i] for i in idx], **_array_kw(), **_lookahead_kw(),
                                **_phase_kw())
        for k, i in enumerate(idx):
            outs[i] = (res["denoised_wav"][k], res["mixed_wav"][k])
    return outs


def normalise(samples):
    """x / (max(abs(x)) + 1e-6) in float64 -> float32 (SN/apply.py:150-155); int16 abs wraps like
    the reference's."""
    with np.errstate(over="ignore"):
        peak = np.max(np.abs(samples)) if len(samples) else 0
    return (samples / (peak + 0.000001)).astype(np.float32)


def trim_to_frames(samples):
    """Drop the tail that does not fill a hop, so that the STFT covers every kept sample
    (SN/apply.py:158-161).  Python's non-negative modulo applies to recordings shorter than one
    window too, exactly as in the reference (300 samples -> 240, which then has no frame at all)."""
    spare = (len(samples) - spec.WIN) % spec.HOP
    return samples[:len(samples) - spare] if spare else samples


def extend_context(samples):
    """Short-context policy: repeat the recording until it yields Noise_Win frames, with the
    reference's repeat rule for noise shorter than speech (SN/apply.py:60-66)."""
    need = spec.MIN_CTX_SAMPLES
    if len(samples) == 0:
        return np.zeros(need, dtype=samples.dtype)
    out = samples
    while need - len(out) > 0:
        out = np.concatenate([out, samples[:need - len(out)]], axis=0)
    return out


_highband_src = {}       # input path -> (the file's channel mean at its own rate, the divisor of its 16 kHz signal)


def _front_end_gpu(eng, path, highband=False):
    """--convert_on gpu: apply.normalise(read_wav_any(path)) computed on the device (resample.front_end).  highband
    (--highband, the input file): also keeps what live.fullband_mix adds back -- the channel mean of the file at its own
    rate, on the int16 scale, and the peak + 1e-6 the 16 kHz signal was divided by."""
    from . import resample
    rate, samples = wavread(path)
    if not highband:
        return resample.front_end(eng, samples, rate, FLAGS.Fs)
    from . import live
    y, peak = resample.front_end(eng, samples, rate, FLAGS.Fs, return_peak=True)
    if not peak > 0:
        raise ValueError("%s: --highband needs a positive peak (a silent file, or the wrapped peak of a mono int16 file "
                         "that reaches -32768)" % path)
    _highband_src[path] = (live.downmix(resample.decode_pcm(samples).T), peak + 0.000001)
    return y


def _handle_signals_gpu(kind, mixedpath, a_path, b_path):
    eng = get_enhancer(kind)

    def context(path):
        if path is None or (os.path.basename(path) == "Silent.wav" and not os.path.exists(path)):
            return np.zeros(spec.MIN_CTX_SAMPLES, dtype=np.float32)
        return extend_context(_front_end_gpu(eng, path))       # (repeating a recording does not change its peak)

    mixed = trim_to_frames(_front_end_gpu(eng, mixedpath, FLAGS.highband is not None))
    if len(mixed) < spec.WIN:
        raise ValueError("%s: shorter than one %d-sample STFT window" % (mixedpath, spec.WIN))
    return context(a_path), context(b_path), mixed


def handle_signals(mixedpath, noisepospath, noisenegpath, kind=None):
    """SN/apply.py:142-167: returns (pos, neg, mixed) float32; wav problems print
    'error in threads' and yield None, like the reference's bare except.  kind: the model whose engine converts the
    files with --convert_on gpu (without it, and by default, everything here is host code)."""
    try:
        if kind is not None and FLAGS.convert_on == "gpu" and getattr(FLAGS, 'convert', False):
            return _handle_signals_gpu(kind, mixedpath, noisepospath, noisenegpath)
        mixedsamples = _reader()(mixedpath)
        noisepossamples = _read_context(noisepospath)
        noisenegsamples = _read_context(noisenegpath)
        mixedsamples = trim_to_frames(normalise(mixedsamples))
        if len(mixedsamples) < spec.WIN:
            raise ValueError("%s: shorter than one %d-sample STFT window" % (mixedpath, spec.WIN))
        return normalise(noisepossamples), normalise(noisenegsamples), mixedsamples
    except Exception:
        print('error in threads')
        print(mixedpath, noisepospath, noisenegpath)
        return None


def _read_context(path):
    if path is None or (os.path.basename(path) == "Silent.wav" and not os.path.exists(path)):
        return np.zeros(spec.MIN_CTX_SAMPLES, dtype=np.int16)
    return extend_context(_reader()(path))


# ------------------------------------------------------------------------------ engine / weights
def _load_weights(kind):
    from . import weights
    if FLAGS.weights == "synthetic":
        return weights.synthetic_weights(kind, 7)
    bundle = DENOISER_BUNDLE if kind == spec.DENOISER else SEPARATOR_BUNDLE
    return weights.load_checkpoint(os.path.join(FLAGS.model_dir, bundle), kind)


def get_engine(kind):
    """The full engine (stage-level entry points, streams, torch tensors): demo / evaluation mode, the sharded
    multi-GPU command line, tests."""
    if kind not in _engines:
        if _lite:
            raise RuntimeError("this process runs the torch-free command-line engine (lite.py); the full engine needs "
                               "PyTorch's HIP runtime loaded first -- use one or the other in a process")
        from . import engine
        _engines[kind] = engine.Engine(kind, _load_weights(kind), device=_device_index)
    return _engines[kind]


def _cache_key(kind):
    from . import blobcache
    if FLAGS.weights == "synthetic":
        return blobcache.key_for_synthetic(kind, 7)
    bundle = DENOISER_BUNDLE if kind == spec.DENOISER else SEPARATOR_BUNDLE
    return blobcache.key_for_checkpoint(os.path.join(FLAGS.model_dir, bundle), kind)


def get_enhancer(kind):
    """What the file / directory command line runs on: an engine with .enhance(mixes, ctx_a, ctx_b, want_mixed).  A
    pre-installed or already built full engine if there is one (set_engine: tests, drivers) or if PyTorch is in the
    process anyway; otherwise -- a fresh `nhans_denoiser` process, the reference's normal use (SN/apply.py:478-527) --
    the torch-free LiteEngine on the cached folded blob: no `import torch` (1.5 s), no folding (3 s), no calibration
    pass."""
    if kind in _engines:
        return _engines[kind]
    if "torch" in sys.modules or int(os.environ.get("WORLD_SIZE", "1")) > 1 or os.environ.get("NHANS_FORCE_TORCH_ENGINE") == "1":
        return get_engine(kind)
    if kind not in _lite:
        os.environ["NHANS_NO_TORCH"] = "1"               # (hip.load: do not pull torch in for its HIP runtime)
        from . import lite
        _lite[kind] = lite.cached_engine(kind, _cache_key(kind) if FLAGS.cache else None, lambda: _load_weights(kind),
                                         device=_device_index, use_cache=FLAGS.cache, timing=TIMING)
    return _lite[kind]


def set_engine(kind, eng):
    """Install a pre-built engine (tests, benchmarks, multi-GPU drivers)."""
    _engines[kind] = eng


# ------------------------------------------------------------------------------ apply_*
def _lookahead_kw():
    """{} at the default, so that an installed engine without the keyword (set_engine) keeps working unasked."""
    L = int(getattr(FLAGS, "lookahead_ms", 10 * spec.LOOKAHEAD)) // 10
    return {} if L == spec.LOOKAHEAD else {"lookahead": L}


def _phase_kw():
    """{} without --phase_iters, for the same reason."""
    n = int(getattr(FLAGS, "phase_iters", 0) or 0)
    return {"phase_iters": n, "phase_alpha": float(getattr(FLAGS, "phase_alpha", 0.0))} if n else {}


def _enhance_files(kind, mixedpath, ctx_a_path, ctx_b_path):
    """-> (denoised_samples, mixed_processed_samples) float32 for one file triple; ctx order is
    resnet_block argument order."""
    import time
    t0 = time.perf_counter()
    sig = handle_array_signals(mixedpath, ctx_a_path, ctx_b_path) if getattr(FLAGS, "array", None) else \
        handle_signals(mixedpath, ctx_a_path, ctx_b_path, kind)
    if sig is None:
        raise RuntimeError("could not read %s / %s / %s" % (mixedpath, ctx_a_path, ctx_b_path))
    ca, cb, mixed = sig
    t1 = time.perf_counter()
    eng = get_enhancer(kind)
    t2 = time.perf_counter()
    if getattr(FLAGS, "array", None):
        (den, mix), = _enhance_arrays(eng, [mixed], [ca], [cb])
        res = {"denoised_wav": [den], "mixed_wav": [mix]}
    elif getattr(FLAGS, "online_ms", None):
        res = _enhance_online(eng, mixedpath, ca, cb, FLAGS.online_ms, mixed if FLAGS.convert_on == "gpu" else None)
    else:
        res = eng.enhance([mixed], [ca], [cb], want_mixed=True, **_lookahead_kw(), **_phase_kw())
    if getattr(FLAGS, "fbank_out", None):
        _write_fbank(eng, mixed, ca, cb, FLAGS.fbank_out)
    if TIMING is not None:
        TIMING.update(read_wavs_s=t1 - t0, engine_s=t2 - t1, enhance_s=time.perf_counter() - t2,
                      engine=type(eng).__name__, audio_s=len(mixed) / float(FLAGS.Fs))
    return res["denoised_wav"][0], res["mixed_wav"][0]


def _write_fbank(eng, mixed, ca, cb, path):
    """--fbank_out: the log-mel features of the denoised clip -- float32 [frames, n_mels], frame g centred on sample
    160 g + 200 of the 16 kHz signal -- from the network's denoised rows on the device (Context.features: a second pass of
    the network, no iSTFT), written with numpy.save.  The same look-ahead as the audio."""
    from . import fbank
    fb = fbank.Filterbank(n_mels=FLAGS.n_mels, scale=FLAGS.mel_scale)
    try:
        feats = eng.features([mixed], [ca], [cb], fb, **_lookahead_kw())[0]
    finally:
        fb.close()
    with open(path, "wb") as f:          # (a file object: numpy.save appends no '.npy' to the name given)
        np.save(f, np.ascontiguousarray(feats, dtype=np.float32))


def _enhance_online(eng, mixedpath, ca, cb, piece_ms, normalised=None):
    """--online_ms: the file normalised with its whole-file peak exactly as offline, then pushed in piece_ms pieces
    through one online stream (online.py); the untrimmed tail is pushed too and dropped by the output contract.
    normalised: the signal the device front end has already converted and normalised (--convert_on gpu)."""
    from . import online
    if normalised is not None:
        x = normalised
    else:
        x = _reader()(mixedpath)
        with np.errstate(over="ignore"):
            peak = np.max(np.abs(x)) if len(x) else 0
        x = online.normalise_fixed(x, peak)
    step = max(1, int(round(piece_ms * FLAGS.Fs / 1000.0)))
    enh = online.OnlineEnhancer(eng, [ca], [cb], want_mixed=True, **_lookahead_kw())
    try:
        den, mix = [], []
        for i in range(0, max(len(x), 1), step):
            last = i + step >= len(x)
            (d, m), = enh.push([x[i:i + step]], end=[last])
            den.append(d)
            mix.append(m)
    finally:
        enh.close()
    return {"denoised_wav": [np.concatenate(den)], "mixed_wav": [np.concatenate(mix)]}


def side_prefix(save_to):
    """Prefix of the side files written next to `save_to`.  The reference cuts 12 characters off the
    output path (`save_to[:-12]`, SN/apply.py:457-470) -- right for its default `.../denoised.wav`
    and for any `<prefix>denoised.wav`, wrong for everything else (for `out/a.wav` the cut eats the
    directory, and in directory mode every clip would overwrite the same three files).  So: the
    reference's cut when the name ends in `denoised.wav`, else `<output without .wav>_`."""
    if os.path.basename(save_to).endswith('denoised.wav'):
        return save_to[:-12]
    return os.path.splitext(save_to)[0] + '_'


_job_rate = {}           # save_to -> (input file's rate, kind): what --output_rate input writes at


def _note_job(kind, mixedpath, save_to):
    if FLAGS.output_rate == "input":
        try:
            _job_rate[save_to] = (int(wavread(mixedpath, mmap=True)[0]), kind)
        except Exception:
            pass                                             # (an unreadable input is reported where it is read)


def _out_rate(save_to):
    """-> (rate, convert): the rate the files of this job are written at and what brings a 16 kHz signal there --
    nothing by default, nhans_resample on the device with --output_rate input and an input at another rate."""
    rate, kind = _job_rate.pop(save_to, (FLAGS.Fs, None)) if FLAGS.output_rate == "input" else (FLAGS.Fs, None)
    if rate == FLAGS.Fs:
        return FLAGS.Fs, lambda x: x
    from . import resample
    eng = get_enhancer(kind)
    return rate, lambda x: resample.resample(eng, [np.asarray(x, dtype=np.float32)], FLAGS.Fs, rate)[0]


_job_high = {}           # save_to -> (kind, x, in_denom): --highband, what _fullband_writer adds to the files of the job


def _note_highband(kind, mixedpath, save_to):
    """--highband, after the input has been through the device front end: binds what it kept to the job's output."""
    if FLAGS.highband is None:
        return
    from . import hip
    rate = _job_rate.get(save_to, (FLAGS.Fs, None))[0]
    if rate not in hip.FULLBAND_RATES:
        raise ValueError("%s: --highband needs an input above 16 kHz (%s Hz); this file is at %d Hz"
                         % (mixedpath, ", ".join(str(r) for r in hip.FULLBAND_RATES), rate))
    _job_high[save_to] = (kind,) + _highband_src.pop(mixedpath)


def _fullband_writer(save_to, rate):
    """None without --highband; with it, full(den, mix, wet) -> the float32 signal at `rate`:
    R(c - G mix) + G x / in_denom, c = den + (mix - den) * wet, on the device (live.fullband_mix)."""
    job = _job_high.pop(save_to, None)
    if job is None:
        return None
    from . import live
    kind, x, in_denom = job
    eng = get_enhancer(kind)
    return lambda den, mix, wet: live.fullband_mix(eng, x, np.asarray(den, dtype=np.float32), np.asarray(mix, dtype=np.float32),
                                                   rate, in_denom, wet=wet, gain=FLAGS.highband, out_dtype=np.float32)


def write_snc_outputs(save_to, denoised_samples, mixed_samples):
    """The four files of SN/apply.py:456-472: denoised, mixed_processed (STFT->iSTFT round trip of
    the input), removed = mixed - denoised, compensated = denoised + removed * factor with the
    factor FLAGS.compensate or, under --ac, snr_est / 20.  Returns (snr_est, factor)."""
    pre = side_prefix(save_to)
    rate, conv = _out_rate(save_to)
    full = _fullband_writer(save_to, rate)
    wavwrite(save_to, rate, full(denoised_samples, mixed_samples, 0.0) if full else conv(denoised_samples))
    wavwrite(pre + 'mixed_processed.wav', rate, conv(mixed_samples))
    removed_samples = mixed_samples - denoised_samples
    wavwrite(pre + 'removed.wav', rate, conv(removed_samples))
    with np.errstate(divide="ignore", invalid="ignore"):
        snr_est = np.mean(np.square(denoised_samples)) / np.mean(np.square(removed_samples))
    print(snr_est)
    print('---------------------------')
    factor = snr_est / 20 if FLAGS.ac else FLAGS.compensate
    compensated_samples = denoised_samples + removed_samples * factor
    wavwrite(pre + 'compensated.wav', rate, full(denoised_samples, mixed_samples, float(factor)) if full and np.isfinite(factor)
             else conv(compensated_samples.astype(np.float32)))
    return snr_est, factor


def apply_snc(mixedpath, pospath, negpath, save_to):
    """Selective noise suppression: keep `pos`-like noise, remove `neg`-like noise
    (SN/apply.py:339-472).  Writes save_to plus the *mixed_processed / *removed / *compensated
    side files (naming: side_prefix)."""
    _note_job(spec.DENOISER, mixedpath, save_to)
    denoised_samples, mixed_samples = _enhance_files(spec.DENOISER, mixedpath, pospath, negpath)
    _note_highband(spec.DENOISER, mixedpath, save_to)
    write_snc_outputs(save_to, denoised_samples, mixed_samples)


def apply_denoiser(mixedpath, negpath, save_to):
    """SN/apply.py:478-481: plain denoising = selective suppression with a silent positive."""
    dir = './audio_examples/'
    pospath = dir + 'Silent.wav'
    apply_snc(mixedpath, pospath, negpath, save_to)


def apply_separator(mixedpath, cleanpath, noisepath, save_to):
    """SS/apply.py:288-397: keep the `cleanpath` (target, --pos) speaker, remove the `noisepath`
    (interferer, --neg) speaker.  resnet_block order is (noise, clean), SS/main.py:205-242."""
    _note_job(spec.SEPARATOR, mixedpath, save_to)
    denoised_samples, mixed_samples = _enhance_files(spec.SEPARATOR, mixedpath, noisepath, cleanpath)
    _note_highband(spec.SEPARATOR, mixedpath, save_to)
    write_separator_outputs(save_to, denoised_samples, mixed_samples)


def write_separator_outputs(save_to, denoised_samples, mixed_samples):
    """SS/apply.py:391-397: the separated target and the round trip of the input."""
    rate, conv = _out_rate(save_to)
    full = _fullband_writer(save_to, rate)
    wavwrite(save_to, rate, full(denoised_samples, mixed_samples, 0.0) if full else conv(denoised_samples))
    wavwrite(side_prefix(save_to) + 'mixed_processed.wav', rate, conv(mixed_samples))


# Audio per nhans_enhance_clips call in directory mode: 4,096 s = 410 ten-second clips = 1.4 GB of
# spectra and waveforms beside the fixed 20 GB stack workspace; a longer job list runs as several calls.
MAX_CALL_SAMPLES = 4096 * Fs

_owns_process_group = False


def _enhance_in_calls(eng, mixes, ca, cb):
    """-> [(denoised, mixed_processed)] per clip, the clips going through the hot path in as few
    ragged calls as MAX_CALL_SAMPLES allows (one for any ordinary directory)."""
    outs, i = [], 0
    while i < len(mixes):
        j, tot = i, 0
        while j < len(mixes) and (j == i or tot + len(mixes[j]) <= MAX_CALL_SAMPLES):
            tot += len(mixes[j])
            j += 1
        res = eng.enhance(mixes[i:j], ca[i:j], cb[i:j], want_mixed=True, **_lookahead_kw(), **_phase_kw())
        outs.extend(zip(res["denoised_wav"], res["mixed_wav"]))
        i = j
    return outs


def apply_batch(kind, jobs):
    """Directory mode (README.md:59-66) as ONE batch: `jobs` is a list of (mixedpath, pospath,
    negpath, save_to).  The recordings go through the hot path in ragged `nhans_enhance_clips`
    calls; under `python -m torch.distributed.run` (WORLD_SIZE > 1) the JOB LIST is sharded over the
    ranks (job i -> rank floor(i*G/N), dist.py): each rank reads, converts and normalises only its
    own block of files and runs it on its own GPU, one all-gather reassembles the waveforms (a job
    whose files could not be read travels as length -1, dist.gather_ragged) and rank 0 writes the files.
    Returns the number of clips written by this rank."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if world > 1:
        import torch
        from . import dist as nd
    lo, hi = nd.shard_bounds(len(jobs), world, rank) if world > 1 else (0, len(jobs))
    sigs = []
    for mixedpath, pospath, negpath, _ in jobs[lo:hi]:
        a_path, b_path = (pospath, negpath) if kind == spec.DENOISER else (negpath, pospath)
        sigs.append(handle_array_signals(mixedpath, a_path, b_path) if getattr(FLAGS, "array", None) else
                    handle_signals(mixedpath, a_path, b_path, kind))    # None: unreadable triple, reported there, skipped
    good = [s for s in sigs if s is not None]
    if world == 1 and not good:
        return 0
    eng = get_enhancer(kind)
    done = iter((_enhance_arrays if getattr(FLAGS, "array", None) else _enhance_in_calls)(
        eng, [s[2] for s in good], [s[0] for s in good], [s[1] for s in good]))
    outs = [None if s is None else next(done) for s in sigs]
    if world > 1:
        import torch.distributed as tdist
        if not tdist.is_initialized():
            global _owns_process_group
            tdist.init_process_group("nccl" if os.environ.get("NHANS_DIST_BACKEND", "nccl") == "nccl" else "gloo")
            _owns_process_group = True
        gather_dev = eng.device if tdist.get_backend() == "nccl" else torch.device("cpu")
        # denoised and round trip travel in one tensor per clip: ONE data all-gather
        local = [None if o is None else torch.from_numpy(np.concatenate(o)).to(gather_dev) for o in outs]
        both = nd.gather_ragged(local, len(jobs), gather_dev)
        if rank != 0:
            return 0
        outs = [None if t is None else (t[:t.numel() // 2].cpu().numpy(), t[t.numel() // 2:].cpu().numpy())
                for t in both]
    written = 0
    for (mixedpath, _, _, save_to), o in zip(jobs, outs):
        if o is None:
            continue
        _note_job(kind, mixedpath, save_to)
        if kind == spec.DENOISER:
            write_snc_outputs(save_to, o[0], o[1])
        else:
            write_separator_outputs(save_to, o[0], o[1])
        written += 1
    return written


def finish_distributed():
    """End of a sharded CLI run: the other ranks wait until rank 0 has written the files, then the
    process group this module created is torn down (no RCCL teardown warnings from early exits)."""
    global _owns_process_group
    if not _owns_process_group:
        return
    import torch.distributed as tdist
    if tdist.is_initialized():
        tdist.barrier()
        tdist.destroy_process_group()
    _owns_process_group = False


# ------------------------------------------------------------------------------ demo / eval mode
def _enhance_after_context(eng, mix_wav, ctx_a_wav, ctx_b_wav, extra_wavs=(), phase_iters=0, phase_alpha=0.0):
    """Shared by apply_demo and the evaluation reader (SN/apply.py:247-266, SN/reader.py:398-409):
    the first Noise_Win frames of the two conditioning signals are the contexts, and the network
    runs on the mixture's frames FROM Noise_Win ON, windowed as a clip of its own (zero rows before
    frame Noise_Win, not the preceding frames).  Uses the stage-level C ABI.  Returns
    (denoised_samples, mixed_samples, [iSTFT of each extra signal's frames from Noise_Win on],
    logits, denoised_logmag).  phase_iters > 0: the denoised samples from phases refined on the denoised rows
    (Engine.phase_refine_rows, from the mixture's); everything else as without."""
    import torch
    dev = eng.device
    wavs = [mix_wav] + list(extra_wavs)
    flat = torch.from_numpy(np.concatenate([np.asarray(w, dtype=np.float32) for w in wavs])).to(dev)
    off = [0]
    for w in wavs:
        off.append(off[-1] + len(w))
    lm, ph = eng.stft_features(flat, off)
    nfr = [int(eng.lib.nhans_num_frames(len(w))) for w in wavs]
    t = nfr[0]
    if t <= Noise_Win:
        raise ValueError("recording has %d frames; more than %d are needed" % (t, Noise_Win))
    ctx = torch.from_numpy(np.concatenate([ctx_a_wav, ctx_b_wav]).astype(np.float32)).to(dev)
    cl, _ = eng.stft_features(ctx, [0, len(ctx_a_wav), len(ctx_a_wav) + len(ctx_b_wav)], Noise_Win, False)
    emb = eng.embed(cl.view(2, Noise_Win, spec.BINS))
    lm_s, ph_s = lm[Noise_Win:t].contiguous(), ph[Noise_Win:t].contiguous()
    n = t - Noise_Win
    logits, den = eng.mask_net(lm_s, [0, n], emb[0:1], emb[1:2])
    den_wav, _ = eng.istft(den, eng.phase_refine_rows(den, ph_s, [0, n], phase_iters, phase_alpha) if phase_iters else ph_s, [0, n])
    mix_rt, _ = eng.istft(lm_s, ph_s, [0, n])
    extras, f0 = [], t
    for k in nfr[1:]:
        w, _ = eng.istft(lm[f0 + Noise_Win:f0 + k].contiguous(), ph[f0 + Noise_Win:f0 + k].contiguous(), [0, k - Noise_Win])
        extras.append(w.cpu().numpy())
        f0 += k
    torch.cuda.synchronize(dev)
    return den_wav.cpu().numpy(), mix_rt.cpu().numpy(), extras, logits.cpu().numpy(), den.cpu().numpy(), lm_s.cpu().numpy()


def _mixed_signals(mix_on, eng, cleanpath, pospath, negpath, snrs=None):
    """mixing.combine_signals on the host (mix_on="host": the code as it always ran) or with the mixing itself on the
    device (mix_on="gpu": Context.mix, the same bits)."""
    from . import mixing
    if mix_on == "host":
        return mixing.combine_signals(read_wav, cleanpath, pospath, negpath, snrs=snrs)
    if mix_on != "gpu":
        raise ValueError("mix_on: 'host' or 'gpu', not %r" % (mix_on,))
    clean, pos, neg = mixing.read_triple(read_wav, cleanpath, pospath, negpath)
    snr_pos, snr_neg = (mixing.SNRS_DENOISER[1], mixing.SNRS_DENOISER[1]) if snrs is None else snrs
    sig, _ = eng.mix([clean], [pos, neg], [(0, 0, 1, snr_pos, snr_neg)])
    return (sig["target"][0], sig["keep"][0], sig["drop"][0], sig["mixture"][0], np.array(snr_pos, dtype=np.int32),
            np.array(snr_neg, dtype=np.int32))


def apply_demo(speechpath, pospath, negpath, save_to, mix_on="host"):
    """Denoiser demo (SN/apply.py:212-336): mix clean speech with a positive and a negative noise
    at 0 dB each, condition on the first 200 frames of the two (scaled) noises, enhance the rest.
    Writes save_to and save_to[:-15] + 'mixed_demo.wav'.  mix_on="gpu": the mixing on the device (the same files)."""
    eng = get_engine(spec.DENOISER)
    _, pos_sig, neg_sig, mixed, _, _ = _mixed_signals(mix_on, eng, speechpath, pospath, negpath)
    den, mix_rt, _, _, _, _ = _enhance_after_context(eng, mixed, pos_sig, neg_sig)
    wavwrite(save_to, FLAGS.Fs, den)
    wavwrite(save_to[:-15] + 'mixed_demo.wav', FLAGS.Fs, mix_rt)


def apply_demo_separator(cleanpath, noisepath, save_to, mix_on="host"):
    """Separator demo (SS/apply.py:179-285): mix two speakers at 0 dB; contexts are the first 200
    frames of the interferer (noise*K -> noisecontextph) and of the target (clean -> cleancontextph).  mix_on="gpu": the
    mixture and the gain K from the device (Context.mix, two-way), noise*K formed on the host as before."""
    from . import mixing
    eng = get_engine(spec.SEPARATOR)
    if mix_on == "host":
        clean, noise_k, mixed, _ = mixing.combine_signals_separator(read_wav, cleanpath, noisepath)
    elif mix_on == "gpu":
        clean = mixing._normalise(read_wav(cleanpath))
        noise = mixing._normalise(read_wav(noisepath))
        clean = clean[:-((len(clean) - spec.WIN) % spec.HOP)]     # sic: unconditional (mixing.combine_signals_separator)
        sig, rec = eng.mix([clean], [noise], [(0, -1, 0, None, 0)])
        mixed, noise_k = sig["mixture"][0], mixing._scaled(rec[0]["g_drop"], noise)
    else:
        raise ValueError("mix_on: 'host' or 'gpu', not %r" % (mix_on,))
    den, mix_rt, _, _, _, _ = _enhance_after_context(eng, mixed, noise_k, clean)
    wavwrite(save_to, FLAGS.Fs, den)
    wavwrite(save_to[:-15] + 'mixed_demo.wav', FLAGS.Fs, mix_rt)


def evaluate_utterance(cleanpath, noisepospath, noisenegpath, dump_dir, modelname='nhans', step=0, scores=False, mix_on="host",
                       stoi=False, bss=False, quality=False, phase_iters=0, phase_alpha=0.0):
    """Evaluation-reader pipeline for one (speech, pos noise, neg noise) triple: SN/reader.py:310-420
    (eval branch, eval_stride 1) + SN/main.py:264-353.  Mixes at the reference's md5-derived SNRs,
    runs the network on frames from context_frames on, writes the reference's five wavs
    `<model>_<step>_<clean>_<pos>_<neg>_<snrp>_<snrn>_{mixed,denoised,target,posNoise,negNoise}.wav`
    and returns the loss of SN/main.py:245-248 for this utterance.  scores=True: -> (that loss, scores): the device figures
    (Engine.score_device / score_rows) of the denoised and of the mixed signal against the target -- waveforms as written,
    row figures from the network's own denoised rows and the mixture's rows against the target's -- their improvement, and
    under "rows" the three row arrays that were scored.  mix_on="gpu": the mixing on the device (the same files and loss).
    stoi=True (with scores): the records also carry STOI and extended STOI of the same waveforms (Engine.stoi_device,
    merged by score.merge_stoi) and the improvement stoi_i and estoi_i; the files and the loss are what they are without it.
    bss=True (with scores): the records also carry SDR, SIR and SAR (Engine.bss_eval_device, merged by score.merge_bss) of
    the same waveforms against the mixing's own target and negative noise -- as mixed, from the first scored sample on --
    and the improvement sdr_i, sir_i and sar_i; the files and the loss are what they are without it.
    quality=True (with scores): the records also carry LLR, cepstral distance and fwSegSNR of the same waveforms
    (Engine.quality_device, merged by score.merge_quality) and the improvement llr_i, llr_95_i, cd_i, cd_95_i (lower is
    better: an improvement is negative) and fwsegsnr_i; the files and the loss are what they are without it.
    phase_iters > 0: the denoised waveform -- the file and every waveform figure of it -- from phases refined by that many
    Griffin-Lim iterations of momentum phase_alpha (Engine.phase_refine_rows); the loss, the row figures and the other four
    files are what they are without it.
    A corpus at several SNR pairs in one pass: evaluate_corpus."""
    from . import mixing
    eng = get_engine(spec.DENOISER)
    target, pos_sig, neg_sig, mixed, snr_pos, snr_neg = _mixed_signals(
        mix_on, eng, cleanpath, noisepospath, noisenegpath, snrs=mixing.eval_snrs(cleanpath))
    den, mix_rt, extras, _, den_lm, mix_lm = _enhance_after_context(eng, mixed, pos_sig, neg_sig,
                                                                    extra_wavs=(target, pos_sig, neg_sig),
                                                                    phase_iters=phase_iters, phase_alpha=phase_alpha)
    import torch
    tgt_lm, _ = eng.stft_features(torch.from_numpy(np.asarray(target, dtype=np.float32)).to(eng.device), [0, len(target)], 0, False)
    tgt_lm = tgt_lm[Noise_Win:].cpu().numpy()
    imp = np.linspace(2, 1, spec.BINS, dtype=np.float32).reshape(1, spec.BINS)
    loss = float(np.mean(np.mean(np.square(den_lm - tgt_lm) * imp, axis=1)))
    os.makedirs(dump_dir, exist_ok=True)
    for kind, w in (('mixed', mix_rt), ('denoised', den), ('target', extras[0]), ('posNoise', extras[1]),
                    ('negNoise', extras[2])):
        wavwrite(_eval_wav_path(dump_dir, modelname, step, (cleanpath, noisepospath, noisenegpath), snr_pos, snr_neg, kind),
                 FLAGS.Fs, w)
    if scores:
        first = Noise_Win * spec.HOP                    # the sample the scored waveforms begin at
        return loss, _utterance_scores(eng, den, mix_rt, extras[0], den_lm, mix_lm, tgt_lm, stoi,
                                       (target[first:], neg_sig[first:]) if bss else None, quality)
    return loss


def phase_ceiling(engine, mixed, target, iters=(0, 8, 32), alpha=0.0):
    """What a perfect mask could reach with and without phase refinement: the clean target's own magnitudes with the
    mixture's phase, refined by each count of `iters` Griffin-Lim iterations on the device (Engine.phase_refine_rows) and
    scored against the target (Engine.score_device).  mixed, target: float32 waveforms of one length, trimmed to whole
    frames -> one record per count: score.FIELDS of the rebuilt waveform against the target, plus "iters" and "inc" (the
    inconsistency of every iteration, float64 [iters]).  The trained model's own rows are not the target's: what the
    iterations gain there is a different figure."""
    import torch
    from . import score
    mixed, target = (np.ascontiguousarray(x, dtype=np.float32) for x in (mixed, target))
    if len(mixed) != len(target):
        raise ValueError("phase_ceiling: mixture and target of one length")
    n = len(target)
    both = torch.from_numpy(np.concatenate([target, mixed])).to(engine.device)
    lm, ph = engine.stft_features(both, [0, n, 2 * n])
    t = lm.shape[0] // 2
    if t == 0:
        raise ValueError("phase_ceiling: fewer than %d samples: no STFT frame" % spec.WIN)
    tlm, mph = lm[:t].contiguous(), ph[t:].contiguous()
    out = []
    for k in iters:
        rph, inc = engine.phase_refine_rows(tlm, mph, [0, t], int(k), alpha, inc=True)
        wav, ooff = engine.istft(tlm, rph, [0, t])
        rec = score.record(engine.score_device(wav, ooff, both[:n].contiguous(), [0, n])[0].cpu().numpy())
        out.append(dict(rec, iters=int(k), inc=inc[0].cpu().numpy()))
    return out


def array_ceiling(engine, x, target, mask, ref=0, loading=1e-6, edge=400):
    """What a mask is worth on an array, with and without the beamformer, on the device: x float32 [n, C] (trimmed to
    whole frames), target: the target's image at channel `ref`, mask: float32 [T, 201] in [0, 1] -> dict of four records
    by score.FIELDS (Engine.score), each against the target over the clip without its first and last `edge` samples --
    "ref": channel `ref` as it is; "mean": the mean of the channels (nhans_channel_mean: what a multi-channel file is
    reduced to today); "mask": the mask alone on channel `ref` (its rows with the log of the mask added, nhans_istft);
    "mvdr": the beamformer's rows (Engine.mvdr_device) through nhans_istft -- and "fallback_bins".  The edges are left
    out because the first and last 240 samples lie under fewer than three frames and are not reconstructed by the
    window pair, which would cost the two estimates that went through it and not the other two."""
    import torch
    from . import hip, mvdr
    x = np.ascontiguousarray(x, dtype=np.float32)
    n, C = x.shape
    T = int(engine.lib.nhans_num_frames(n))
    if T < 1 or (T - 1) * spec.HOP + spec.WIN != n or len(target) != n:
        raise ValueError("array_ceiling: clip and target of one length, trimmed to whole frames")
    if n <= 2 * edge:
        raise ValueError("array_ceiling: nothing left between the edges")
    m = np.ascontiguousarray(mask, dtype=np.float32)
    planes = torch.from_numpy(mvdr.planes(x)).to(engine.device)
    mask_t = torch.from_numpy(m).to(engine.device)
    bf = engine.mvdr_device(planes, [0, n], C, mask_t, ref=ref, loading=loading)
    wav_bf, _ = engine.istft(bf["logmag"], bf["phase"], [0, T])
    # the mask alone: one channel through the same filter is that channel (w = 1), with the log of the mask as its gain
    gain = torch.from_numpy(np.log(np.maximum(mvdr.mask_values(m), 1e-8)).astype(np.float32)).to(engine.device)
    one = engine.mvdr_device(planes[ref * n:(ref + 1) * n].contiguous(), [0, n], 1, mask_t, gain_t=gain)
    wav_mask, _ = engine.istft(one["logmag"], one["phase"], [0, T])
    mean = torch.empty(n, dtype=torch.float32, device=engine.device)
    hip.check(engine.lib.nhans_channel_mean(engine.handle, hip.ptr(planes), C, n, hip.ptr(mean), engine._stream()))
    cut = lambda w: np.ascontiguousarray(np.asarray(w, dtype=np.float32)[edge:n - edge])
    est = [cut(x[:, ref]), cut(mean.cpu().numpy()), cut(wav_mask.cpu().numpy()), cut(wav_bf.cpu().numpy())]
    recs = engine.score(est, [cut(target)] * 4)
    out = dict(zip(("ref", "mean", "mask", "mvdr"), recs))
    out["fallback_bins"] = int(bf["records"][0, 3].item())
    return out


def _eval_wav_path(dump_dir, modelname, step, triple, snr_pos, snr_neg, kind):
    base = [os.path.basename(p)[:-4] for p in triple]
    return os.path.join(dump_dir, '{}_{}_{}_{}_{}_{}_{}_{}.wav'.format(modelname, step, base[0], base[1], base[2], snr_pos, snr_neg, kind))


def evaluate_corpus(triples, snrs=None, lookahead=spec.LOOKAHEAD, dump_dir=None, per_frame=False, modelname='nhans', step=0,
                    stoi=False, bss=False, quality=False, phase_iters=0, phase_alpha=0.0):
    """evaluate_utterance(scores=True) for a corpus in one pass.  triples: (cleanpath, pospath, negpath) each; snrs: the
    (snr_pos, snr_neg) pairs applied to every triple (None: the triple's own mixing.eval_snrs).  The files are read,
    normalised and trimmed on the host and uploaded once; the mixtures of all (triple, SNR pair) jobs (Engine.mix_device),
    their STFTs, the tower over the 2 J context images, the stack over every job's frames from Noise_Win on, the iSTFTs
    and the scoring run on the device over all jobs together, and only the records come back -- with dump_dir also the
    five waveforms per job, written under evaluate_utterance's names.  lookahead as in Engine.enhance; a saturated f16x3
    batch is redone in f32 as everywhere (context.redo_saturated_in_f32).
    -> one dict per job, triple after triple: "triple", "snr_pos", "snr_neg", "loss" (the denoised rows' loss as the
    device forms it: the "loss" of evaluate_utterance's scores, bit for bit), "denoised", "mixed", "improvement" (as
    evaluate_utterance's scores) and "mix" (the job's mixing record); per_frame=True: plus "per_frame" in "denoised" and
    "mixed", float64 [frames, 3] as Context.score's.  stoi=True: STOI and extended STOI in the same pass, as
    evaluate_utterance(scores=True, stoi=True) merges them, bit for bit; only their records come back.  bss=True: SDR, SIR
    and SAR against each job's own target and negative noise, which the mixing left in HBM, likewise.  quality=True: LLR,
    cepstral distance and fwSegSNR in the same pass, as evaluate_utterance(scores=True, quality=True) merges them, bit for
    bit.  phase_iters, phase_alpha: as evaluate_utterance's, the refinement of all jobs in the same pass."""
    from . import context, mixing, score
    eng = get_engine(spec.DENOISER)
    speech, noises, jobs, meta = [], [], [], []
    for ti, triple in enumerate(triples):
        clean, pos, neg = mixing.read_triple(read_wav, *triple)
        t = int(eng.lib.nhans_num_frames(len(clean)))
        if t <= Noise_Win:
            raise ValueError("%s: the mixture has %d frames; more than %d are needed" % (triple[0], t, Noise_Win))
        speech.append(clean)
        noises += [pos, neg]
        for snr_pos, snr_neg in ([mixing.eval_snrs(triple[0])] if snrs is None else snrs):
            jobs.append((ti, 2 * ti, 2 * ti + 1, snr_pos, snr_neg))
            meta.append({"triple": tuple(triple), "snr_pos": snr_pos, "snr_neg": snr_neg})
    if not jobs:
        return []
    sp_t, sp_off = eng._dev(speech)
    nz_t, nz_off = eng._dev(noises)
    sig, off, mix_rec = eng.mix_device(sp_t, sp_off, nz_t, nz_off, jobs)
    dump = dump_dir is not None
    res = eng._with_lookahead(lookahead, lambda: context.redo_saturated_in_f32(
        eng, lambda: _corpus_device(eng, sig, off, per_frame, dump, stoi, bss, quality, (int(phase_iters), float(phase_alpha)))))
    eng._sync()
    mix_rec = mix_rec.cpu().numpy()
    down = {k: v.cpu().numpy() for k, v in res["records"].items()}
    frames = {k: v.cpu().numpy() for k, v in res["frames"].items()}
    waves = {k: v.cpu().numpy() for k, v in res["waves"].items()}
    roff, ooff = res["roff"], res["ooff"]
    if dump:
        os.makedirs(dump_dir, exist_ok=True)
    out = []
    for j, m in enumerate(meta):
        r = dict(m)
        for name in ("denoised", "mixed"):
            r[name] = dict(score.record(down[name + "_wave"][j]), **score.row_record(down[name + "_rows"][j]))
            if stoi:
                r[name] = score.merge_stoi(r[name], score.stoi_record(down[name + "_stoi"][j]))
            if bss:
                r[name] = score.merge_bss(r[name], score.bss_record(down[name + "_bss"][j]))
            if quality:
                r[name] = score.merge_quality(r[name], score.quality_record(down[name + "_quality"][j]))
            if per_frame:
                r[name]["per_frame"] = frames[name][roff[j]:roff[j + 1]].copy()
        r["loss"] = r["denoised"]["loss"]
        r["improvement"] = score.improvement(r["mixed"], r["denoised"])
        r["mix"] = dict(zip(mixing.RECORD_FIELDS, (float(v) for v in mix_rec[j])))
        for kind, w in waves.items():
            wavwrite(_eval_wav_path(dump_dir, modelname, step, m["triple"], m["snr_pos"], m["snr_neg"], kind), FLAGS.Fs,
                     w[ooff[j]:ooff[j + 1]])
        out.append(r)
    return out


def _corpus_device(eng, sig, off, per_frame, dump, stoi=False, bss=False, quality=False, refine=(0, 0.0)):
    """The launches of evaluate_corpus after the mixing, everything in HBM: job j's signals are [off[j], off[j + 1]) of
    sig's tensors -> device records (and, for a dump, waveforms)."""
    import torch
    from . import context
    J = len(off) - 1
    nfr = [int(eng.lib.nhans_num_frames(off[j + 1] - off[j])) for j in range(J)]
    foff = context.offsets(nfr)
    roff = context.offsets(t - Noise_Win for t in nfr)

    def rest(rows):
        """rows [Noise_Win, t) of every job, one after the other"""
        return torch.cat([rows[foff[j] + Noise_Win:foff[j + 1]] for j in range(J)]).contiguous()

    lm, ph = eng.stft_features(sig["mixture"], off)
    tlm, tph = eng.stft_features(sig["target"], off)
    kl, _ = eng.stft_features(sig["keep"], off, Noise_Win, False)
    dl, _ = eng.stft_features(sig["drop"], off, Noise_Win, False)
    emb = eng.embed(torch.cat([kl, dl]).view(2 * J, Noise_Win, spec.BINS))
    lm_s, ph_s, tlm_s, tph_s = rest(lm), rest(ph), rest(tlm), rest(tph)
    _, den = eng.mask_net(lm_s, roff, emb[:J], emb[J:], want_logits=False)
    den_wav, ooff = eng.istft(den, eng.phase_refine_rows(den, ph_s, roff, *refine) if refine[0] else ph_s, roff)
    mix_rt, _ = eng.istft(lm_s, ph_s, roff)
    tgt_wav, _ = eng.istft(tlm_s, tph_s, roff)
    records, frames = {}, {}
    # the sources of BSS Eval: job j's target and drop signals as mixed, from the first scored sample on (a clip is cut to
    # the samples the estimate has, so a source's range may run on into the next job's)
    soff = [o + Noise_Win * spec.HOP for o in off[:-1]] + [off[-1]]
    for name, wav, rows in (("denoised", den_wav, den), ("mixed", mix_rt, lm_s)):
        w = eng.score_device(wav, ooff, tgt_wav, ooff, per_frame=per_frame)
        r = eng.score_rows(rows, tlm_s, roff, per_frame=per_frame, frames_out=w[1] if per_frame else None)
        records[name + "_wave"], records[name + "_rows"] = (w[0], r[0]) if per_frame else (w, r)
        if stoi:
            records[name + "_stoi"] = eng.stoi_device(wav, ooff, tgt_wav, ooff)
        if bss:
            records[name + "_bss"] = eng.bss_eval_device(wav, ooff, [(sig["target"], soff), (sig["drop"], soff)])
        if quality:
            records[name + "_quality"] = eng.quality_device(wav, ooff, tgt_wav, ooff)
        if per_frame:
            frames[name] = r[1]
    waves = {}
    if dump:
        waves = {"mixed": mix_rt, "denoised": den_wav, "target": tgt_wav}
        for kind, x in (("posNoise", sig["keep"]), ("negNoise", sig["drop"])):
            xl, xp = eng.stft_features(x, off)
            waves[kind], _ = eng.istft(rest(xl), rest(xp), roff)
    return {"records": records, "frames": frames, "waves": waves, "roff": roff, "ooff": ooff}


def _utterance_scores(eng, den, mix_rt, target, den_lm, mix_lm, tgt_lm, stoi=False, bss_sources=None, quality=False):
    import torch
    from . import score
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(eng.device)
    tw, tr = dev(target), dev(tgt_lm)
    out = {}
    for name, wav, rows in (("denoised", den, den_lm), ("mixed", mix_rt, mix_lm)):
        w = eng.score_device(dev(wav), [0, len(wav)], tw, [0, len(target)])
        r = eng.score_rows(dev(rows), tr, [0, len(tgt_lm)])
        out[name] = dict(score.record(w.cpu().numpy()[0]), **score.row_record(r.cpu().numpy()[0]))
        if stoi:
            st = eng.stoi_device(dev(wav), [0, len(wav)], tw, [0, len(target)])
            out[name] = score.merge_stoi(out[name], score.stoi_record(st.cpu().numpy()[0]))
        if bss_sources is not None:
            b = eng.bss_eval_device(dev(wav), [0, len(wav)], [(dev(x), [0, len(x)]) for x in bss_sources])
            out[name] = score.merge_bss(out[name], score.bss_record(b.cpu().numpy()[0]))
        if quality:
            qr = eng.quality_device(dev(wav), [0, len(wav)], tw, [0, len(target)])
            out[name] = score.merge_quality(out[name], score.quality_record(qr.cpu().numpy()[0]))
    out["improvement"] = score.improvement(out["mixed"], out["denoised"])
    out["rows"] = {"denoised": den_lm, "mixed": mix_lm, "target": tgt_lm}
    return out


# ------------------------------------------------------------------------------ CLI
def _parse(argv, prog):
    p = argparse.ArgumentParser(prog=prog)
    p.add_argument('--input', default=FLAGS.input)
    p.add_argument('--neg', default=FLAGS.neg)
    p.add_argument('--pos', default=FLAGS.pos)
    p.add_argument('--output', default=FLAGS.output)
    p.add_argument('--compensate', type=float, default=0.0)
    p.add_argument('--ac', action='store_true')
    p.add_argument('--weights', default=FLAGS.weights, choices=['checkpoint', 'synthetic'])
    p.add_argument('--model_dir', default=FLAGS.model_dir)
    p.add_argument('--no-cache', dest='cache', action='store_false', default=True,
                   help='fold the weights in this process instead of reading / writing the folded-blob cache '
                        '($NHANS_CACHE_DIR or ~/.cache/nhans_amd: blobcache.py)')
    p.add_argument('--timing', action='store_true', help='print the seconds of each start-up step as JSON on stderr')
    p.add_argument('--no-convert', dest='convert', action='store_false', default=True,
                   help='reject inputs that are not 16 kHz int16 PCM (in-tree reference behaviour) '
                        'instead of converting them (packaged-tool behaviour, README.md:42)')
    p.add_argument('--online_ms', type=float, default=None,
                   help='file mode only: push the input through the online (live-stream) path in pieces of this many '
                        'milliseconds; the files written are byte-identical to the offline run')
    p.add_argument('--convert_on', default='host', choices=['host', 'gpu'],
                   help='where files that are not 16 kHz int16 PCM are converted and all files normalised: host (scipy, '
                        'the default) or gpu (the device rate converter, rates of nhans_amd.resample.RATES)')
    p.add_argument('--output_rate', default='16000', choices=['16000', 'input'],
                   help='input: write the output files at the input file\'s rate (converted back on the device)')
    p.add_argument('--highband', type=float, default=None, metavar='G',
                   help='file mode with --output_rate input --convert_on gpu, input above 16 kHz: the denoised and the '
                        'compensated file also carry the input\'s own band above 8 kHz, times G (0 ... 4; 1: as it came in) '
                        '-- the 16 kHz network path has none.  A multi-channel input gives the band of its channel mean')
    p.add_argument('--lookahead_ms', type=float, default=10.0 * spec.LOOKAHEAD,
                   help='future audio every output frame may use: a multiple of 10 in 0 ... 170 (default 170, all 17 frames '
                        'of the window).  Less is what a live stream of that look-ahead would have produced -- latency '
                        '10 ms per frame + 25 ms -- at a cost in quality that depends on the trained model')
    p.add_argument('--phase_iters', type=int, default=0, metavar='N',
                   help='Griffin-Lim iterations on the denoised rows, from the mixture\'s phase, before the denoised file is rebuilt '
                        '(0 ... 256; default 0: the mixture\'s phase as it is; offline only)')
    p.add_argument('--phase_alpha', type=float, default=0.0, metavar='A', help='momentum of --phase_iters, 0 <= A < 1 (default 0)')
    p.add_argument('--array', default=None, choices=['mvdr'],
                   help='a multi-channel input keeps its channels: the network\'s mask, from the mean of the channels, picks the '
                        'spatial covariances of speech and noise, and an MVDR beamformer is put on the channels on the device '
                        '(file and directory mode; default: the mean of the channels, as always)')
    p.add_argument('--array_ref', type=int, default=0, metavar='R', help='reference channel of --array (default 0)')
    p.add_argument('--array_post', default='none', choices=['none', 'mask', 'net'],
                   help='what follows the beamformer of --array: nothing, the same mask, or a second pass of the network (default none)')
    p.add_argument('--fbank_out', default=None, metavar='PATH.npy',
                   help='file mode only: also write the log-mel filterbank features of the denoised signal (float32 '
                        '[frames, n_mels], 25 ms / 10 ms frames, numpy.save) computed on the device from the network\'s '
                        'denoised rows; the audio files are what they are without the flag')
    p.add_argument('--n_mels', type=int, default=80, help='bands of --fbank_out, 1 ... 128 (default 80), 0 - 8000 Hz')
    p.add_argument('--mel_scale', default='htk', choices=['htk', 'slaney'], help='mel scale of --fbank_out (default htk)')
    p.add_argument('--score_against', default=None, metavar='TARGET',
                   help='a clean target of the input -- a wav in file mode, a directory paired by file name in directory '
                        'mode: the denoised file and the mixed round trip are scored against it on the device (SI-SDR, SNR, '
                        'segmental SNR, the reference\'s loss, log-spectral distance) and the scores written as JSON; the '
                        'audio files are what they are without the flag')
    p.add_argument('--score_out', default=None, metavar='PATH.json', help='where the scores of --score_against go (default: stdout)')
    p.add_argument('--stoi', action='store_true',
                   help='with --score_against: also STOI and extended STOI of the same files against the target, converted to '
                        '10 kHz and computed on the device; the audio files are what they are without the flag')
    p.add_argument('--quality', action='store_true',
                   help='with --score_against: also the log-likelihood ratio and the cepstral distance of the LPC models (lower '
                        'is better) and the frequency-weighted segmental SNR of the same files against the target, computed on '
                        'the device; the audio files are what they are without the flag')
    p.add_argument('--bss', action='store_true',
                   help='with --score_against and --interferer: also SDR, SIR and SAR (BSS Eval, filters of 512 taps) of the same '
                        'files against the target and the interferer, computed on the device; the audio files are what they '
                        'are without the flag')
    p.add_argument('--interferer', default=None, metavar='FILE',
                   help='for --bss: the signal that was to be removed -- the noise, or the other speaker; a wav in file mode, a '
                        'directory paired by file name in directory mode.  It needs no peak scaling: the decomposition does not '
                        'change when a source is scaled, or filtered by up to 512 taps')
    p.add_argument('--align_ms', type=float, default=None, metavar='MS',
                   help='with --score_against, for a target that is not sample-aligned with the input: the delay of the '
                        'denoised file against the target is estimated on the device within MS milliseconds either way '
                        '(0 < MS <= 1000; whole samples, positive: the files are late) and taken out of the denoised file, '
                        'the mixed round trip and the target (and the --interferer) before they are scored; the scores '
                        'gain delay_samples and align_rho per file; the audio files are what they are without the flag')
    p.add_argument('--align_drift', action='store_true',
                   help='with --align_ms, for a target recorded on another clock: the delay of the denoised file against '
                        'the target is tracked over the file around the one --align_ms finds, a line delay + drift fitted '
                        'to it, and the denoised file and the mixed round trip resampled onto the target\'s clock on the '
                        'device before they are scored (the target and the --interferer are cut to the same range); the '
                        'scores gain delay_samples (real), drift_ppm and drift_ok per file; the audio files are what they '
                        'are without the flag')
    a = p.parse_args(argv)
    if a.align_drift and a.align_ms is None:
        p.error('--align_drift needs --align_ms MS')
    if a.align_ms is not None:
        if a.score_against is None:
            p.error('--align_ms needs --score_against TARGET')
        if not 0.0 < a.align_ms <= 1000.0:
            p.error('--align_ms must be in 0 < MS <= 1000; got %g' % a.align_ms)
    if a.bss != (a.interferer is not None):
        p.error('--bss and --interferer FILE go together')
    if a.bss and a.score_against is None:
        p.error('--bss needs --score_against TARGET')
    if a.score_out is not None and a.score_against is None:
        p.error('--score_out needs --score_against TARGET')
    if a.stoi and a.score_against is None:
        p.error('--stoi needs --score_against TARGET')
    if a.quality and a.score_against is None:
        p.error('--quality needs --score_against TARGET')
    if a.score_against is not None:
        if a.output_rate == 'input':
            p.error('--score_against scores the 16 kHz files; it does not combine with --output_rate input')
        if a.convert_on == 'gpu':
            p.error('--score_against reads and scales the target on the host; it does not combine with --convert_on gpu')
        if os.path.isdir(a.input) != os.path.isdir(a.score_against):
            p.error('--score_against must be a directory when --input is one, and a file when it is a file')
        if os.path.isdir(a.input):
            for name in sorted(os.listdir(a.input)):
                if name.lower().endswith('.wav') and not os.path.isfile(os.path.join(a.score_against, name)):
                    p.error('--score_against: %s has no target of the same name in %s' % (name, a.score_against))
        elif not os.path.isfile(a.score_against):
            p.error('--score_against: %s is not a file' % a.score_against)
        if a.bss:
            if os.path.isdir(a.input) != os.path.isdir(a.interferer):
                p.error('--interferer must be a directory when --input is one, and a file when it is a file')
            if os.path.isdir(a.input):
                for name in sorted(os.listdir(a.input)):
                    if name.lower().endswith('.wav') and not os.path.isfile(os.path.join(a.interferer, name)):
                        p.error('--interferer: %s has no interferer of the same name in %s' % (name, a.interferer))
            elif not os.path.isfile(a.interferer):
                p.error('--interferer: %s is not a file' % a.interferer)
    if a.fbank_out is not None:
        if os.path.isdir(a.input):
            p.error('--fbank_out works on one input file; %s is a directory' % a.input)
        if not 1 <= a.n_mels <= 128:
            p.error('--n_mels must be in 1 ... 128; got %d' % a.n_mels)
    if not 0 <= a.lookahead_ms <= 10 * spec.LOOKAHEAD or a.lookahead_ms != 10 * int(a.lookahead_ms // 10):
        p.error('--lookahead_ms must be a multiple of 10 in 0 ... %d (one 10 ms frame of look-ahead each); got %g'
                % (10 * spec.LOOKAHEAD, a.lookahead_ms))
    a.lookahead_ms = int(a.lookahead_ms)
    if a.highband is not None:
        if not 0.0 <= a.highband <= 4.0:
            p.error('--highband must be in 0 ... 4; got %g' % a.highband)
        if os.path.isdir(a.input) or int(os.environ.get("WORLD_SIZE", "1")) > 1:
            p.error('--highband works on one input file (directory mode and sharded runs write 16 kHz batches)')
        if a.output_rate != 'input' or a.convert_on != 'gpu' or not a.convert:
            p.error('--highband needs --output_rate input --convert_on gpu (and no --no-convert): the band is added at the '
                    'input file\'s own rate, on the device')
    if a.array is None:
        if a.array_ref != 0 or a.array_post != 'none':
            p.error('--array_ref and --array_post need --array mvdr')
    else:
        for flag, on in (('--online_ms', a.online_ms is not None), ('--convert_on gpu', a.convert_on == 'gpu'),
                         ('--highband', a.highband is not None), ('--fbank_out', bool(a.fbank_out)),
                         ('a sharded run', int(os.environ.get("WORLD_SIZE", "1")) > 1)):
            if on:
                p.error('--array does not go with %s' % flag)
        names = [os.path.join(a.input, n) for n in sorted(os.listdir(a.input)) if n.lower().endswith('.wav')] \
            if os.path.isdir(a.input) else [a.input]
        for path in names:
            try:
                shape = wavread(path, mmap=True)[1].shape
            except Exception:
                continue                                     # (an unreadable input is reported where it is read)
            C = shape[1] if len(shape) == 2 else 1
            if C < 2:
                p.error('--array needs inputs with more than one channel; %s is mono' % path)
            if C > 8:
                p.error('--array takes up to 8 channels; %s has %d' % (path, C))
            if not 0 <= a.array_ref < C:
                p.error('--array_ref must be in 0 ... %d for %s; got %d' % (C - 1, path, a.array_ref))
    if not 0 <= a.phase_iters <= 256:
        p.error('--phase_iters must be in 0 ... 256; got %d' % a.phase_iters)
    if not 0.0 <= a.phase_alpha < 1.0:
        p.error('--phase_alpha must be in [0, 1); got %g' % a.phase_alpha)
    if a.phase_iters and a.online_ms is not None:
        p.error('--phase_iters does not go with --online_ms: every iteration reaches two frames further into the future')
    if a.online_ms is not None:
        if a.online_ms <= 0:
            p.error('--online_ms must be positive')
        if os.path.isdir(a.input):
            p.error('--online_ms works on one input file; %s is a directory (directory mode is offline batches)' % a.input)
    for k, v in vars(a).items():
        setattr(FLAGS, k, v)
    return a


def _pairs(a):
    """File mode or directory mode: in directory mode inputs and conditioning recordings are
    paired by identical file name (README.md:59-66)."""
    if os.path.isdir(a.input):
        os.makedirs(a.output, exist_ok=True)
        for name in sorted(os.listdir(a.input)):
            if not name.lower().endswith('.wav'):
                continue
            pick = lambda d: os.path.join(d, name) if os.path.isdir(d) else d
            yield os.path.join(a.input, name), pick(a.pos), pick(a.neg), os.path.join(a.output, name)
    else:
        yield a.input, a.pos, a.neg, a.output


def _run_cli(kind, a):
    global TIMING
    import time
    t0 = time.perf_counter()
    TIMING = {} if getattr(a, "timing", False) else None
    try:
        _run_cli_jobs(kind, a)
    finally:
        if TIMING is not None:
            import json
            TIMING["run_cli_s"] = time.perf_counter() - t0
            TIMING["torch_imported"] = "torch" in sys.modules
            sys.stderr.write("nhans timing: " + json.dumps(TIMING) + "\n")
            TIMING = None


def _run_cli_jobs(kind, a):
    jobs = list(_pairs(a))
    if os.path.isdir(a.input) or int(os.environ.get("WORLD_SIZE", "1")) > 1:
        _bind_rank_device()
        try:
            apply_batch(kind, jobs)
            if getattr(a, "score_against", None) and int(os.environ.get("RANK", "0")) == 0:
                _score_jobs(kind, a, jobs)
        finally:
            finish_distributed()
    else:
        for mixed, pos, neg, out in jobs:
            (apply_snc if kind == spec.DENOISER else apply_separator)(mixed, pos, neg, out)
        if getattr(a, "score_against", None):
            _score_jobs(kind, a, jobs)


def scaled_target(mixedpath, targetpath):
    """--score_against: the target read as the input is read (16 kHz on the host) and put on the scale the network saw
    the input on -- multiplied by the INPUT's peak factor 1 / (max|input| + 1e-6), as the reference's mixing puts a target
    on the mixture's scale -- float32."""
    x = _reader()(mixedpath)
    with np.errstate(over="ignore"):
        peak = np.max(np.abs(x)) if len(x) else 0
    return (_reader()(targetpath) / (peak + 0.000001)).astype(np.float32)


def _score_jobs(kind, a, jobs):
    """--score_against, after the files are written: per job the 16 kHz denoised file and the mixed round trip, as
    written, against the scaled target over their common prefix, in ONE Context.score call; JSON to --score_out or
    stdout: {"files": {input path: {"denoised", "mixed", "improvement"}}, "skipped": [...]} and, in directory mode, "mean".
    --align_ms: one Context.align call first, each denoised file against its target within round(16 MS) samples; a file's
    delay is taken out of both of its signals alike -- the two are sample-aligned by construction -- and out of the
    interferer as out of the target, and the file's entry gains "delay_samples" and "align_rho".
    --align_drift: one Context.align_drift call instead, the line of each denoised file against its target; a file's line is
    warped out of both of its signals alike and the target and the interferer are cut to the warp's range; the file's
    entry gains "delay_samples" (real), "drift_ppm", "drift_ok" and "align_rho"."""
    import json
    from . import score
    directory = os.path.isdir(a.input)
    done, skipped, est, tgt, interf = [], [], [], [], []
    bss = getattr(a, "bss", False)
    for mixedpath, _, _, save_to in jobs:
        mp = side_prefix(save_to) + 'mixed_processed.wav'
        if not (os.path.exists(save_to) and os.path.exists(mp)):
            skipped.append(mixedpath)                       # (reported where it was read: no output to score)
            continue
        t = scaled_target(mixedpath, os.path.join(a.score_against, os.path.basename(mixedpath)) if directory else a.score_against)
        est += [wavread(save_to)[1], wavread(mp)[1]]
        tgt += [t, t]
        if bss:
            x = _reader()(os.path.join(a.interferer, os.path.basename(mixedpath)) if directory else a.interferer).astype(np.float32)
            interf += [x, x]
        done.append(mixedpath)
    align_ms, found = getattr(a, "align_ms", None), None
    lines = None
    if align_ms is not None and est and getattr(a, "align_drift", False):
        eng = get_enhancer(kind)
        lines = eng.align_drift(est[0::2], tgt[0::2], max_lag=int(round(16 * align_ms)))
        est, tgt, interf = eng._drift_pairs(est, tgt, interf if bss else None, [l for l in lines for _ in (0, 1)])
    elif align_ms is not None and est:
        found = get_enhancer(kind).align(est[0::2], tgt[0::2], max_lag=int(round(16 * align_ms)))
    recs = get_enhancer(kind).score(est, tgt, stoi=getattr(a, "stoi", False), bss=interf if bss else None,
                                    quality=getattr(a, "quality", False),
                                    delays=[r["delay"] for r in found for _ in (0, 1)] if found else None) if est else []
    files = {}
    for i, path in enumerate(done):
        den, mix = recs[2 * i], recs[2 * i + 1]
        files[path] = {"denoised": den, "mixed": mix, "improvement": score.improvement(mix, den)}
        if found:
            files[path].update(delay_samples=found[i]["delay"], align_rho=found[i]["rho"])
        if lines:
            l = lines[i]
            files[path].update(delay_samples=l["delay"] if l["fit_ok"] else l["delay_int"], drift_ppm=l["drift_ppm"],
                               drift_ok=l["fit_ok"], align_rho=l["rho"])
    out = {"files": files, "skipped": skipped}
    if directory and files:
        out["mean"] = {k: score.mean_of([f[k] for f in files.values()]) for k in ("denoised", "mixed", "improvement")}
    text = json.dumps(out, indent=1, sort_keys=True)
    if a.score_out:
        with open(a.score_out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)


def _bind_rank_device():
    """One process per GPU under torch.distributed.run: LOCAL_RANK picks the device.  Runs before
    anything has touched the GPU."""
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if local and all(k not in _engines for k in (spec.DENOISER, spec.SEPARATOR)):
        import torch
        torch.cuda.set_device(local)
        global _device_index
        _device_index = local


def main(argv=None):
    """`nhans_denoiser` (setup.py:46).  `--input/--output` (and optionally `--pos/--neg`) may be
    directories: files are paired by name and processed as one batch; launched through
    `python -m torch.distributed.run --nproc-per-node N -m ...` the batch is sharded over N GPUs."""
    _run_cli(spec.DENOISER, _parse(argv, 'nhans_denoiser'))


def main_separator(argv=None):
    """`nhans_separator` (setup.py:48)."""
    _run_cli(spec.SEPARATOR, _parse(argv, 'nhans_separator'))


if __name__ == '__main__':
    main(sys.argv[1:])
