"""ctypes binding of libnhans_hip.so (C ABI in include/nhans_hip.h).

There is no CPU fallback: if the shared library is missing or fails to load, every use raises.
"""
import ctypes
import json
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
# ($NHANS_LIB: another build of the same library for a same-box A/B of two kernels -- a developer convenience of this
# Python binding; the library itself reads no environment)
LIB_PATH = os.environ.get("NHANS_LIB") or os.path.join(_HERE, "csrc", "libnhans_hip.so")

DENOISER, SEPARATOR = 0, 1
KIND_CODE = {"denoiser": DENOISER, "separator": SEPARATOR}

EXPORTS = [
    "nhans_abi_version", "nhans_last_error", "nhans_num_frames", "nhans_create", "nhans_create_ex", "nhans_destroy",
    "nhans_set_option", "nhans_workspace_bytes", "nhans_stft_features", "nhans_embed",
    "nhans_mask_net", "nhans_istft", "nhans_enhance_clips", "nhans_debug_block_output",
    "nhans_profile_json", "nhans_profile_reset", "nhans_take_status", "nhans_debug_launch_probe", "nhans_crc32c",
    "nhans_debug_mfma_ceiling", "nhans_set_activation_exponents", "nhans_get_activation_exponents",
    "nhans_get_activation_amax", "nhans_online_open", "nhans_online_push", "nhans_online_out_counts",
    "nhans_online_rewind", "nhans_online_close", "nhans_online_open_slots", "nhans_online_restart",
    "nhans_online_set_context", "nhans_online_set_embeddings", "nhans_resample_out_count", "nhans_resample_emitted",
    "nhans_resample_taps", "nhans_resample", "nhans_peak_normalise", "nhans_channel_mean", "nhans_resampler_open", "nhans_resampler_set_peak",
    "nhans_resampler_push", "nhans_resampler_out_counts", "nhans_resampler_restart", "nhans_resampler_close",
    "nhans_debug_activation", "nhans_debug_tower_activation",
    "nhans_live_emitted", "nhans_live_open_slots", "nhans_live_restart", "nhans_live_set_context",
    "nhans_live_set_embeddings", "nhans_live_set_wet", "nhans_live_out_counts", "nhans_live_push", "nhans_live_rewind",
    "nhans_live_close", "nhans_online_set_lookahead", "nhans_lookahead_live_emitted", "nhans_lookahead_live_set",
    "nhans_capture_plan", "nhans_capture_enable", "nhans_capture_context", "nhans_capture_embeddings",
    "nhans_capture_live_enable", "nhans_capture_live_context", "nhans_capture_live_embeddings",
    "nhans_level_hops", "nhans_level_live_enable", "nhans_level_live_auto", "nhans_level_live_read",
    "nhans_level_live_gains", "nhans_level_gains",
]
PCM_INT16, PCM_FLOAT32 = 0, 1
RESAMPLE_QUANTISE = 1
NORMALISE_WRAP_INT16 = 1
LIVE_WET = 1
CAPTURE_SAMPLES = 32240
CAPTURE_A, CAPTURE_B = 0, 1
CAPTURE_NORMALISE = 1
ESHORT = -4
LEVEL_MAX_WINDOW = 256
STATUS_SATURATED = 1
NUM_ACTIVATIONS = 25
ABI_VERSION = 5

_lib = None


class NhansError(RuntimeError):
    pass


def load():
    """Load the HIP library once; raises NhansError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NhansError("%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                         "or `make -C n-hans_amd/csrc` (there is no CPU fallback)" % LIB_PATH)
    # With torch in the process its bundled libamdhip64.so.7 must be THE HIP runtime (two runtimes in one process do not
    # share devices or streams): torch is imported first unless the caller has said this process stays torch-free
    # (NHANS_NO_TORCH=1, set by the single-process command line: lite.py) -- importing it costs more than a one-file call.
    if os.environ.get("NHANS_NO_TORCH") != "1" or "torch" in sys.modules:
        import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    vp, i64p = ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)
    lib.nhans_abi_version.restype = ctypes.c_int
    lib.nhans_last_error.restype = ctypes.c_char_p
    lib.nhans_num_frames.restype = ctypes.c_int64
    lib.nhans_num_frames.argtypes = [ctypes.c_int64]
    lib.nhans_create.argtypes = [ctypes.c_int, vp, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(vp)]
    lib.nhans_create_ex.argtypes = [ctypes.c_int, vp, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int,
                                    ctypes.POINTER(vp)]
    lib.nhans_destroy.argtypes = [vp]
    lib.nhans_destroy.restype = None
    lib.nhans_set_option.argtypes = [vp, ctypes.c_char_p, ctypes.c_int64]
    lib.nhans_workspace_bytes.argtypes = [vp, ctypes.c_int64, ctypes.c_int]
    lib.nhans_workspace_bytes.restype = ctypes.c_size_t
    lib.nhans_stft_features.argtypes = [vp, vp, i64p, ctypes.c_int, ctypes.c_int, vp, vp, vp]
    lib.nhans_embed.argtypes = [vp, vp, ctypes.c_int, vp, vp]
    lib.nhans_mask_net.argtypes = [vp, vp, i64p, ctypes.c_int, vp, vp, vp, vp, vp]
    lib.nhans_istft.argtypes = [vp, vp, vp, i64p, ctypes.c_int, i64p, vp, vp]
    lib.nhans_enhance_clips.argtypes = [vp, vp, i64p, ctypes.c_int, vp, i64p, vp, i64p, vp, vp, vp, vp, vp, vp, vp]
    lib.nhans_debug_block_output.argtypes = [vp, vp, i64p, ctypes.c_int, vp, vp, ctypes.c_int64, ctypes.c_int,
                                             ctypes.c_int, vp, vp]
    lib.nhans_profile_json.argtypes = [vp, ctypes.c_char_p, ctypes.c_size_t]
    lib.nhans_profile_reset.argtypes = [vp]
    lib.nhans_take_status.argtypes = [vp, ctypes.POINTER(ctypes.c_int), vp]
    lib.nhans_debug_launch_probe.argtypes = [ctypes.c_size_t, vp]
    lib.nhans_debug_mfma_ceiling.argtypes = [ctypes.c_double, vp, ctypes.POINTER(ctypes.c_double),
                                             ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)]
    lib.nhans_debug_mfma_ceiling.restype = ctypes.c_int
    lib.nhans_set_activation_exponents.argtypes = [vp, ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    lib.nhans_get_activation_exponents.argtypes = [vp, ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    lib.nhans_get_activation_amax.argtypes = [vp, ctypes.POINTER(ctypes.c_float), ctypes.c_int]
    # (online enhancement; a build from before it -- $NHANS_LIB in a same-box A/B -- has none of these: build() and
    # tests/test_host.py check that the library in the tree exports every symbol of the header)
    online = hasattr(lib, "nhans_online_open")
    if online:
        ip = ctypes.POINTER(ctypes.c_int)
        lib.nhans_online_open.argtypes = [vp, ctypes.c_int, vp, i64p, vp, i64p, ctypes.c_int, vp, ctypes.POINTER(vp)]
        lib.nhans_online_push.argtypes = [vp, vp, i64p, ip, vp, vp, i64p, i64p, vp]
        lib.nhans_online_out_counts.argtypes = [vp, i64p, ip, i64p]
        lib.nhans_online_rewind.argtypes = [vp]
        lib.nhans_online_close.argtypes = [vp]
        lib.nhans_online_close.restype = None
    # (slot reuse and live conditioning came one change after the online functions: the library of that one commit,
    # as $NHANS_LIB in an A/B against it, has the five above and not these)
    slots = online and hasattr(lib, "nhans_online_open_slots")
    if slots:
        lib.nhans_online_open_slots.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp, ctypes.POINTER(vp)]
        lib.nhans_online_restart.argtypes = [vp, ctypes.c_int]
        lib.nhans_online_set_context.argtypes = [vp, ctypes.c_int, vp, ctypes.c_int64, vp, ctypes.c_int64, vp, i64p]
        lib.nhans_online_set_embeddings.argtypes = [vp, ctypes.c_int, vp, vp, vp, i64p]
    # (sample-rate conversion came after the slots; the library of an earlier commit as $NHANS_LIB has none of these)
    rates = hasattr(lib, "nhans_resample")
    if rates:
        ip = ctypes.POINTER(ctypes.c_int)
        lib.nhans_resample_out_count.argtypes = [ctypes.c_int64, ctypes.c_int, ctypes.c_int]
        lib.nhans_resample_out_count.restype = ctypes.c_int64
        lib.nhans_resample_emitted.argtypes = [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int]
        lib.nhans_resample_emitted.restype = ctypes.c_int64
        lib.nhans_resample_taps.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.c_int]
        lib.nhans_resample.argtypes = [vp, vp, ctypes.c_int, i64p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp,
                                       i64p, vp]
        lib.nhans_peak_normalise.argtypes = [vp, vp, i64p, ctypes.c_int, ctypes.c_int, vp, vp]
        lib.nhans_channel_mean.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int64, vp, vp]
        lib.nhans_channel_mean.restype = ctypes.c_int
        lib.nhans_resampler_open.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                             ctypes.POINTER(vp)]
        lib.nhans_resampler_set_peak.argtypes = [vp, ctypes.c_double]
        lib.nhans_resampler_push.argtypes = [vp, vp, i64p, ip, vp, i64p, i64p, vp]
        lib.nhans_resampler_out_counts.argtypes = [vp, i64p, ip, i64p]
        lib.nhans_resampler_restart.argtypes = [vp, ctypes.c_int]
        lib.nhans_resampler_close.argtypes = [vp]
        lib.nhans_resampler_close.restype = None
        for name in ("nhans_resample_taps", "nhans_resample", "nhans_peak_normalise", "nhans_resampler_open",
                     "nhans_resampler_set_peak", "nhans_resampler_push", "nhans_resampler_out_counts",
                     "nhans_resampler_restart"):
            getattr(lib, name).restype = ctypes.c_int
    # (the taps on every stored tensor came after the rate converter: looked up by symbol like the groups above)
    if hasattr(lib, "nhans_debug_activation"):
        lib.nhans_debug_activation.argtypes = [vp, vp, i64p, ctypes.c_int, vp, vp, ctypes.c_int64, ctypes.c_int,
                                               ctypes.c_int, vp, vp]
        lib.nhans_debug_tower_activation.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, vp, vp]
        lib.nhans_debug_activation.restype = lib.nhans_debug_tower_activation.restype = ctypes.c_int
    # (live PCM sessions came after those: looked up by symbol as well)
    if hasattr(lib, "nhans_live_push"):
        ip = ctypes.POINTER(ctypes.c_int)
        lib.nhans_live_emitted.argtypes = [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int]
        lib.nhans_live_emitted.restype = ctypes.c_int64
        lib.nhans_live_open_slots.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int,
                                              ctypes.c_int, ctypes.c_double, ctypes.c_int, vp, ctypes.POINTER(vp)]
        lib.nhans_live_restart.argtypes = [vp, ctypes.c_int]
        lib.nhans_live_set_context.argtypes = [vp, ctypes.c_int, vp, ctypes.c_int64, vp, ctypes.c_int64, vp, i64p]
        lib.nhans_live_set_embeddings.argtypes = [vp, ctypes.c_int, vp, vp, vp, i64p]
        lib.nhans_live_set_wet.argtypes = [vp, ctypes.c_double]
        lib.nhans_live_out_counts.argtypes = [vp, i64p, ip, i64p]
        lib.nhans_live_push.argtypes = [vp, vp, i64p, ip, vp, i64p, i64p, vp]
        lib.nhans_live_rewind.argtypes = [vp]
        lib.nhans_live_close.argtypes = [vp]
        lib.nhans_live_close.restype = None
        for name in ("nhans_live_open_slots", "nhans_live_restart", "nhans_live_set_context", "nhans_live_set_embeddings",
                     "nhans_live_set_wet", "nhans_live_out_counts", "nhans_live_push", "nhans_live_rewind"):
            getattr(lib, name).restype = ctypes.c_int
    # (the selectable look-ahead came after the live sessions: looked up by symbol; the option "lookahead" of such an
    # older library is unknown to it and nhans_set_option says so)
    if hasattr(lib, "nhans_online_set_lookahead"):
        lib.nhans_online_set_lookahead.argtypes = [vp, ctypes.c_int, ctypes.c_int]
        lib.nhans_online_set_lookahead.restype = ctypes.c_int
        lib.nhans_lookahead_live_set.argtypes = [vp, ctypes.c_int, ctypes.c_int]
        lib.nhans_lookahead_live_set.restype = ctypes.c_int
        lib.nhans_lookahead_live_emitted.argtypes = [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
        lib.nhans_lookahead_live_emitted.restype = ctypes.c_int64
    # (conditioning captured from a slot's own stream came after the look-ahead: looked up by symbol)
    if hasattr(lib, "nhans_capture_context"):
        ip = ctypes.POINTER(ctypes.c_int)
        lib.nhans_capture_plan.argtypes = [ctypes.c_int64, ctypes.c_int64, i64p]
        for obj in ("", "live_"):
            getattr(lib, "nhans_capture_%senable" % obj).argtypes = [vp, vp]
            getattr(lib, "nhans_capture_%scontext" % obj).argtypes = [vp, ctypes.c_int, ip, ip, ctypes.c_int, vp, i64p]
            getattr(lib, "nhans_capture_%sembeddings" % obj).argtypes = [vp, ctypes.c_int, vp, vp, vp]
        for name in EXPORTS:
            if name.startswith("nhans_capture_"):
                getattr(lib, name).restype = ctypes.c_int
    # (the level meter of a live session came after the captured conditioning: looked up by symbol)
    if hasattr(lib, "nhans_level_hops"):
        lib.nhans_level_hops.argtypes = [ctypes.c_int64, ctypes.c_int]
        lib.nhans_level_live_enable.argtypes = [vp, vp]
        lib.nhans_level_live_auto.argtypes = [vp, ctypes.c_int, ctypes.c_double]
        lib.nhans_level_live_read.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_double), vp]
        lib.nhans_level_live_gains.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_float), ctypes.c_int64, vp]
        lib.nhans_level_gains.argtypes = [vp, vp, vp, i64p, ctypes.c_int, ctypes.c_int, ctypes.c_double, vp, vp, vp]
        for name in EXPORTS:
            if name.startswith("nhans_level_"):
                getattr(lib, name).restype = ctypes.c_int
        lib.nhans_level_hops.restype = lib.nhans_level_live_gains.restype = ctypes.c_int64
    lib.nhans_crc32c.argtypes = [ctypes.c_uint32, vp, ctypes.c_size_t]
    lib.nhans_crc32c.restype = ctypes.c_uint32
    for name in ("nhans_create", "nhans_create_ex", "nhans_set_option", "nhans_stft_features", "nhans_embed", "nhans_mask_net",
                 "nhans_istft", "nhans_enhance_clips", "nhans_debug_block_output", "nhans_profile_json",
                 "nhans_profile_reset", "nhans_take_status", "nhans_debug_launch_probe",
                 "nhans_set_activation_exponents", "nhans_get_activation_exponents", "nhans_get_activation_amax") + (
                 ("nhans_online_open", "nhans_online_push", "nhans_online_out_counts", "nhans_online_rewind") if online else ()) + (
                 ("nhans_online_open_slots", "nhans_online_restart", "nhans_online_set_context",
                  "nhans_online_set_embeddings") if slots else ()):
        getattr(lib, name).restype = ctypes.c_int
    if lib.nhans_abi_version() != ABI_VERSION:
        raise NhansError("libnhans_hip.so ABI version mismatch")
    _lib = lib
    return lib


def check(rc):
    if rc < 0:
        err = NhansError("libnhans_hip: %s (code %d)" % (load().nhans_last_error().decode(), rc))
        err.code = rc
        raise err
    return rc


def i64_array(values):
    arr = (ctypes.c_int64 * len(values))(*[int(v) for v in values])
    return arr


def ptr(t):
    """Device pointer of a contiguous torch tensor (None -> NULL)."""
    if t is None:
        return None
    assert t.is_contiguous()
    return ctypes.c_void_p(t.data_ptr())


def mfma_ceiling(seconds, stream=None):
    """-> dict(sustained_tflops, first_launch_tflops, launches): the f16 MFMA rate the current device
    holds at its power cap (nhans_debug_mfma_ceiling)."""
    sus, first, n = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_int(0)
    check(load().nhans_debug_mfma_ceiling(float(seconds), stream, ctypes.byref(sus), ctypes.byref(first), ctypes.byref(n)))
    return {"sustained_tflops": sus.value, "first_launch_tflops": first.value, "launches": n.value}


def profile_dict(handle):
    lib = load()
    n = lib.nhans_profile_json(handle, None, 0)
    buf = ctypes.create_string_buffer(n + 1)
    lib.nhans_profile_json(handle, buf, n + 1)
    return json.loads(buf.value.decode())
