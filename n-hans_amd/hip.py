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

_int, _i64, _dbl, _vp = ctypes.c_int, ctypes.c_int64, ctypes.c_double, ctypes.c_void_p
_size, _str = ctypes.c_size_t, ctypes.c_char_p
_ip, _i64p, _vpp = ctypes.POINTER(_int), ctypes.POINTER(_i64), ctypes.POINTER(_vp)
_fp, _dp = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(_dbl)
# name -> (restype, argtypes) of every function of include/nhans_hip.h, in the header's order (tests/test_host.py holds
# the names, the argument counts and the return types to the header).  Device pointers, handles and hipStream_t are
# void*; host arrays carry their element type.
SIGNATURES = {
    "nhans_abi_version": (_int, []),
    "nhans_last_error": (_str, []),
    "nhans_num_frames": (_i64, [_i64]),
    "nhans_create": (_int, [_int, _vp, _size, _int, _vpp]),
    "nhans_create_ex": (_int, [_int, _vp, _size, _int, _ip, _int, _vpp]),
    "nhans_destroy": (None, [_vp]),
    "nhans_set_option": (_int, [_vp, _str, _i64]),
    "nhans_set_activation_exponents": (_int, [_vp, _ip, _int]),
    "nhans_get_activation_exponents": (_int, [_vp, _ip, _int]),
    "nhans_get_activation_amax": (_int, [_vp, _fp, _int]),
    "nhans_workspace_bytes": (_size, [_vp, _i64, _int]),
    "nhans_stft_features": (_int, [_vp, _vp, _i64p, _int, _int, _vp, _vp, _vp]),
    "nhans_embed": (_int, [_vp, _vp, _int, _vp, _vp]),
    "nhans_mask_net": (_int, [_vp, _vp, _i64p, _int, _vp, _vp, _vp, _vp, _vp]),
    "nhans_istft": (_int, [_vp, _vp, _vp, _i64p, _int, _i64p, _vp, _vp]),
    "nhans_enhance_clips": (_int, [_vp, _vp, _i64p, _int, _vp, _i64p, _vp, _i64p, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "nhans_debug_block_output": (_int, [_vp, _vp, _i64p, _int, _vp, _vp, _i64, _int, _int, _vp, _vp]),
    "nhans_debug_activation": (_int, [_vp, _vp, _i64p, _int, _vp, _vp, _i64, _int, _int, _vp, _vp]),
    "nhans_debug_tower_activation": (_int, [_vp, _vp, _int, _int, _vp, _vp]),
    "nhans_take_status": (_int, [_vp, _ip, _vp]),
    "nhans_debug_launch_probe": (_int, [_size, _vp]),
    "nhans_debug_mfma_ceiling": (_int, [_dbl, _vp, _dp, _dp, _ip]),
    "nhans_debug_row_classes": (_int, [_int, _int, _int, _int, _ip, _int]),
    "nhans_debug_builtin_batch": (_int, [_fp, _fp, _fp, _i64p]),
    "nhans_crc32c": (ctypes.c_uint32, [ctypes.c_uint32, _vp, _size]),
    # online enhancement
    "nhans_online_open": (_int, [_vp, _int, _vp, _i64p, _vp, _i64p, _int, _vp, _vpp]),
    "nhans_online_open_slots": (_int, [_vp, _int, _int, _vp, _vpp]),
    "nhans_online_restart": (_int, [_vp, _int]),
    "nhans_online_set_context": (_int, [_vp, _int, _vp, _i64, _vp, _i64, _vp, _i64p]),
    "nhans_online_set_embeddings": (_int, [_vp, _int, _vp, _vp, _vp, _i64p]),
    "nhans_online_push": (_int, [_vp, _vp, _i64p, _ip, _vp, _vp, _i64p, _i64p, _vp]),
    "nhans_online_out_counts": (_int, [_vp, _i64p, _ip, _i64p]),
    "nhans_online_rewind": (_int, [_vp]),
    "nhans_online_set_lookahead": (_int, [_vp, _int, _int]),
    "nhans_online_close": (None, [_vp]),
    # sample-rate conversion and the file front end
    "nhans_resample_out_count": (_i64, [_i64, _int, _int]),
    "nhans_resample_emitted": (_i64, [_i64, _int, _int, _int]),
    "nhans_resample_taps": (_int, [_int, _int, _dp, _int]),
    "nhans_resample": (_int, [_vp, _vp, _int, _i64p, _int, _int, _int, _int, _vp, _i64p, _vp]),
    "nhans_peak_normalise": (_int, [_vp, _vp, _i64p, _int, _int, _vp, _vp]),
    "nhans_channel_mean": (_int, [_vp, _vp, _int, _i64, _vp, _vp]),
    "nhans_resampler_open": (_int, [_vp, _int, _int, _int, _int, _int, _vpp]),
    "nhans_resampler_set_peak": (_int, [_vp, _dbl]),
    "nhans_resampler_push": (_int, [_vp, _vp, _i64p, _ip, _vp, _i64p, _i64p, _vp]),
    "nhans_resampler_out_counts": (_int, [_vp, _i64p, _ip, _i64p]),
    "nhans_resampler_restart": (_int, [_vp, _int]),
    "nhans_resampler_close": (None, [_vp]),
    # live PCM sessions
    "nhans_live_emitted": (_i64, [_i64, _int, _int, _int]),
    "nhans_live_open_slots": (_int, [_vp, _int, _int, _int, _dbl, _int, _int, _dbl, _int, _vp, _vpp]),
    "nhans_live_restart": (_int, [_vp, _int]),
    "nhans_live_set_context": (_int, [_vp, _int, _vp, _i64, _vp, _i64, _vp, _i64p]),
    "nhans_live_set_embeddings": (_int, [_vp, _int, _vp, _vp, _vp, _i64p]),
    "nhans_live_set_wet": (_int, [_vp, _dbl]),
    "nhans_live_out_counts": (_int, [_vp, _i64p, _ip, _i64p]),
    "nhans_live_push": (_int, [_vp, _vp, _i64p, _ip, _vp, _i64p, _i64p, _vp]),
    "nhans_lookahead_live_emitted": (_i64, [_i64, _int, _int, _int, _int]),
    "nhans_lookahead_live_set": (_int, [_vp, _int, _int]),
    "nhans_live_rewind": (_int, [_vp]),
    "nhans_live_close": (None, [_vp]),
    # conditioning captured from a slot's own stream
    "nhans_capture_plan": (_int, [_i64, _i64, _i64p]),
    "nhans_capture_enable": (_int, [_vp, _vp]),
    "nhans_capture_context": (_int, [_vp, _int, _ip, _ip, _int, _vp, _i64p]),
    "nhans_capture_embeddings": (_int, [_vp, _int, _vp, _vp, _vp]),
    "nhans_capture_live_enable": (_int, [_vp, _vp]),
    "nhans_capture_live_context": (_int, [_vp, _int, _ip, _ip, _int, _vp, _i64p]),
    "nhans_capture_live_embeddings": (_int, [_vp, _int, _vp, _vp, _vp]),
    # level meter and automatic compensation
    "nhans_level_hops": (_i64, [_i64, _int]),
    "nhans_level_live_enable": (_int, [_vp, _vp]),
    "nhans_level_live_auto": (_int, [_vp, _int, _dbl]),
    "nhans_level_live_read": (_int, [_vp, _int, _dp, _vp]),
    "nhans_level_live_gains": (_i64, [_vp, _int, _fp, _i64, _vp]),
    "nhans_level_gains": (_int, [_vp, _vp, _vp, _i64p, _int, _int, _dbl, _vp, _vp, _vp]),
    # live sessions on interleaved frames
    "nhans_interleaved_live_open": (_int, [_vp, _int, _int, _int, _int, _int, _int, _dbl, _int, _int, _dbl, _int, _vp, _vpp]),
    "nhans_interleaved_live_out_counts": (_int, [_vp, _i64p, _ip, _i64p]),
    "nhans_interleaved_live_push": (_int, [_vp, _vp, _i64p, _ip, _vp, _i64p, _i64p, _vp]),
    # filterbank features
    "nhans_fbank_design": (_int, [_int, _dbl, _dbl, _int, _int, _dp]),
    "nhans_fbank_open": (_int, [_vp, _dp, _int, _int, _dbl, _vp, _vpp]),
    "nhans_fbank_close": (None, [_vp]),
    "nhans_fbank_rows": (_int, [_vp, _vp, _i64, _vp, _vp]),
    "nhans_fbank_online_attach": (_int, [_vp, _vp, _int]),
    "nhans_fbank_online_read": (_i64, [_vp, _int, _int, _vp, _i64, _i64p, _vp]),
    "nhans_fbank_live_attach": (_int, [_vp, _vp, _int]),
    "nhans_fbank_live_read": (_i64, [_vp, _int, _int, _vp, _i64, _i64p, _vp]),
    # full-band live output
    "nhans_fullband_hold_samples": (_i64, [_int]),
    "nhans_fullband_live_enable": (_int, [_vp, _vp]),
    "nhans_fullband_live_set_gain": (_int, [_vp, _int, _dbl]),
    "nhans_fullband_mix": (_int, [_vp, _vp, _int, _i64p, _vp, _vp, _i64p, _int, _int, _dbl, _dbl, _vp, _dbl, _dbl, _int, _vp,
                                  _i64p, _vp]),
    # scoring against a clean target
    "nhans_score_wave": (_int, [_vp, _vp, _i64p, _vp, _i64p, _int, _vp, _vp, _vp]),
    "nhans_score_rows": (_int, [_vp, _vp, _vp, _i64p, _int, _vp, _vp, _vp]),
    # mixing at a chosen SNR
    "nhans_mix_snr_factor": (_int, [_dbl, _dp]),
    "nhans_mix": (_int, [_vp, _vp, _i64p, _int, _vp, _i64p, _int, _ip, _ip, _ip, _dp, _dp, _int, _vp, _vp, _vp, _vp, _i64p, _vp,
                         _vp]),
    # STOI and extended STOI against a clean target
    "nhans_stoi_out_count": (_i64, [_i64]),
    "nhans_stoi_resample": (_int, [_vp, _vp, _i64p, _int, _vp, _i64p, _vp]),
    "nhans_stoi": (_int, [_vp, _vp, _i64p, _vp, _i64p, _int, _vp, _vp, _vp]),
    # BSS Eval against target and interferer (the two tables are host arrays: of device pointers, of host offset arrays)
    "nhans_bss_eval": (_int, [_vp, _vp, _i64p, _vpp, ctypes.POINTER(_i64p), _int, _int, _int, _vp, _vp, _vp]),
    # delay estimation and the cut to the common part
    "nhans_align": (_int, [_vp, _vp, _i64p, _vp, _i64p, _int, _int, _vp, _vp, _vp]),
    "nhans_align_common": (_i64, [_i64, _i64, _i64]),
    "nhans_align_cut": (_int, [_vp, _vp, _i64p, _vp, _i64p, _int, _i64p, _vp, _vp, _i64p, _vp]),
    # LLR, cepstral distance and frequency-weighted segmental SNR against a clean target (the band matrix is a host array)
    "nhans_quality": (_int, [_vp, _vp, _i64p, _vp, _i64p, _int, _dp, _int, _vp, _vp, _vp]),
    "nhans_quality_lpc": (_int, [_vp, _vp, _i64p, _vp, _i64p, _int, _vp, _vp]),
    "nhans_quality_tables": (_int, [_dp, _dp]),
    # drift-aware alignment: the delay tracked over a clip, the line fit and the warp (the lines are host arrays)
    "nhans_drift_table": (_int, [_dp, _dp]),
    "nhans_drift_segments": (_i64, [_i64]),
    "nhans_drift_range": (_int, [_i64, _i64, _dbl, _dbl, _i64p, _i64p]),
    "nhans_drift_fit": (_int, [_dp, _int, _dbl, _dbl, _dp]),
    "nhans_drift_track": (_int, [_vp, _vp, _i64p, _vp, _i64p, _int, _dp, _dp, _int, _vp, _vp, _vp]),
    "nhans_drift_warp": (_int, [_vp, _vp, _i64p, _i64p, _int, _dp, _dp, _vp, _i64p, _vp]),
    # phase refinement: Griffin-Lim iterations after the mask
    "nhans_phase_set_alpha": (_int, [_vp, _dbl]),
    "nhans_phase_project": (_int, [_vp, _vp, _vp, _i64p, _int, _vp, _vp, _vp]),
    "nhans_phase_refine": (_int, [_vp, _vp, _vp, _i64p, _int, _int, _dbl, _vp, _vp, _vp]),
    # mask-driven MVDR beamforming of multi-channel clips
    "nhans_mvdr_spectra": (_int, [_vp, _vp, _i64p, _int, _int, _vp, _vp, _vp, _vp]),
    "nhans_mvdr_weights": (_int, [_vp, _vp, _vp, _i64p, _int, _int, _int, _dbl, _int, _vp, _vp, _vp, _vp]),
    "nhans_mvdr_apply": (_int, [_vp, _vp, _vp, _vp, _i64p, _int, _int, _vp, _vp, _vp, _vp, _vp]),
    "nhans_mvdr": (_int, [_vp, _vp, _i64p, _int, _int, _vp, _int, _dbl, _int, _vp, _vp, _vp, _vp, _vp, _vp]),
    "nhans_profile_json": (_int, [_vp, _str, _size]),
    "nhans_profile_reset": (_int, [_vp]),
}
EXPORTS = list(SIGNATURES)
PCM_INT16, PCM_FLOAT32 = 0, 1
RESAMPLE_QUANTISE = 1
NORMALISE_WRAP_INT16 = 1
LIVE_WET = 1
CAPTURE_SAMPLES = 32240
CAPTURE_A, CAPTURE_B = 0, 1
CAPTURE_NORMALISE = 1
ESHORT = -4
LEVEL_MAX_WINDOW = 256
INTERLEAVED_DOWNMIX, INTERLEAVED_SPLIT = 0, 1
INTERLEAVED_MAX_CHANNELS = 8
FBANK_MAX_OUT, FBANK_MAX_SPAN = 128, 8192
FBANK_HTK, FBANK_SLANEY = 0, 1
FBANK_NORM_NONE, FBANK_NORM_SLANEY = 0, 1
FBANK_MIXED = 1
FULLBAND_RATES = (22050, 24000, 32000, 44100, 48000, 88200, 96000)
SCORE_FIELDS, SCORE_ROW_FIELDS = 16, 8
SCORE_TILE = 2560                           # samples per workgroup of score.hip (kScoreTile)
MIX_FIELDS = 8
STOI_FIELDS = 8
BSS_FIELDS = 16
BSS_MAX_FILTER = 512
BSS_CORR_TILE = 2048                        # samples per workgroup of bsseval.hip's correlation launch (kBssCorrTile)
ALIGN_FIELDS = 8
ALIGN_MAX_LAG = 16000
ALIGN_TILE, ALIGN_LAG_BLOCK = 2048, 2048    # samples per tile and lags per workgroup of align.hip (kAlignTile, kAlignLagBlock)
DRIFT_FIELDS, DRIFT_FIT_FIELDS = 8, 6
DRIFT_TAPS, DRIFT_PHASES, DRIFT_BLOCK, DRIFT_HOP, DRIFT_MAX_RADIUS = 16, 512, 4096, 2048, 1024
DRIFT_TILE, DRIFT_FINE, DRIFT_WARP_TILE = 2048, 32, 1024    # samples per fma chain, fine positions per sample, outputs per workgroup of drift.hip
QUALITY_FIELDS, QUALITY_LPC_FIELDS = 16, 72
QUALITY_FRAME, QUALITY_HOP, QUALITY_ORDER, QUALITY_FFT, QUALITY_BINS = 480, 120, 16, 512, 257
QUALITY_BANDS, QUALITY_MAX_BANDS = 25, 32
QUALITY_LPC_TILE, QUALITY_BAND_TILE = 7, 2  # frames per workgroup of quality.hip's LPC and band launches (kQualityLpcTile, kQualityBandTile)
PHASE_MAX_ITERS = 256
MVDR_MAX_CHANNELS, MVDR_FIELDS, MVDR_LOGGAIN = 8, 6, 1
MVDR_RUN = 32                               # frames per workgroup of mvdr.hip's filter (kMvdrRun)
PHASE_RUN = 20                              # frames per run of phase.hip's projection (kPhaseRun)
MIX_TILE = 2048                             # samples per workgroup and per staging buffer of mix.hip (kMixTile)
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
    # (per symbol: a build from an older commit -- $NHANS_LIB in a same-box A/B -- loads with the functions it has;
    # build() and tests/test_host.py check that the library in the tree exports every symbol of the header)
    for name, (restype, argtypes) in SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
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


def dbl_array(values):
    values = [float(v) for v in values]
    return (ctypes.c_double * len(values))(*values)


def drift_range(ne, nt, a, b):
    """-> (u_lo, u_hi): the target samples a warp by the line (a, b) covers (nhans_drift_range, host only)"""
    lo, hi = ctypes.c_int64(0), ctypes.c_int64(0)
    check(load().nhans_drift_range(int(ne), int(nt), float(a), float(b), ctypes.byref(lo), ctypes.byref(hi)))
    return lo.value, hi.value


def drift_fit(rows, rho_min, trim):
    """rows of NHANS_DRIFT_FIELDS doubles, one clip's segments -> dict by score.DRIFT_FIT_FIELDS (nhans_drift_fit, host only)"""
    import numpy as np
    from . import score
    flat = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, DRIFT_FIELDS)
    out = (ctypes.c_double * DRIFT_FIT_FIELDS)()
    check(load().nhans_drift_fit(flat.ctypes.data_as(_dp), len(flat), float(rho_min), float(trim), out))
    return score.drift_fit_record(list(out))


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


def builtin_batch():
    """-> (mixtures, ctx_a, ctx_b): two float32 numpy arrays each -- the batch nhans_create calibrates the activation
    exponents on (nhans_debug_builtin_batch, host only)."""
    import numpy as np
    lib = load()
    n = (ctypes.c_int64 * 2)()
    check(lib.nhans_debug_builtin_batch(None, None, None, n))
    mix, ca, cb = np.zeros(2 * n[0], np.float32), np.zeros(2 * n[1], np.float32), np.zeros(2 * n[1], np.float32)
    as_fp = lambda a: a.ctypes.data_as(_fp)
    check(lib.nhans_debug_builtin_batch(as_fp(mix), as_fp(ca), as_fp(cb), n))
    return tuple([a[:len(a) // 2], a[len(a) // 2:]] for a in (mix, ca, cb))


def profile_dict(handle):
    lib = load()
    n = lib.nhans_profile_json(handle, None, 0)
    buf = ctypes.create_string_buffer(n + 1)
    lib.nhans_profile_json(handle, buf, n + 1)
    return json.loads(buf.value.decode())
