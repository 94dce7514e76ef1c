"""Filterbank features of log-magnitude rows (include/nhans_hip.h: nhans_fbank_*): log-mel frames of the enhanced signal
straight from the network's denoised rows, on the device -- offline (Engine.features, Engine.fbank_rows) and live
(online.Slots.enable_fbank / features).  The framing is the network's own: 400-sample periodic Hann window, hop 160,
201 bins 40 Hz apart; frame g is centred on sample 160 g + 200 of the 16 kHz signal.

Filterbank holds the matrix (designed by the library in double, or the caller's own) and opens it per engine on demand;
reference() restates the header's definition in float64 numpy.  No torch here: the torch-free engine uses it too."""
import ctypes
import weakref

import numpy as np

from . import hip, spec

SCALES = {"htk": hip.FBANK_HTK, "slaney": hip.FBANK_SLANEY}
NORMS = {None: hip.FBANK_NORM_NONE, "slaney": hip.FBANK_NORM_SLANEY}
MAX_EXPONENT = 88.0        # p = exp(min(power * x, 88)): the header's clamp, inactive over the network's rows


def design(n_mels=80, f_min=0.0, f_max=8000.0, scale="htk", norm=None):
    """-> (W float64 [n_mels, 201], bands that are empty after float32 rounding): nhans_fbank_design, host only."""
    if scale not in SCALES:
        raise ValueError("scale: 'htk' or 'slaney' (got %r)" % (scale,))
    if norm not in NORMS:
        raise ValueError("norm: None or 'slaney' (got %r)" % (norm,))
    W = np.zeros((max(int(n_mels), 0), spec.BINS), dtype=np.float64)
    empty = hip.check(hip.load().nhans_fbank_design(int(n_mels), float(f_min), float(f_max), SCALES[scale], NORMS[norm],
                                                    W.ctypes.data_as(ctypes.POINTER(ctypes.c_double))))
    return W, empty


class Filterbank:
    """n_mels triangular bands between f_min and f_max Hz on the mel scale `scale` ('htk' | 'slaney'), norm None or
    'slaney' -- librosa's and torchaudio's definitions --, applied to power-`power` spectra (1 | 2) with the result
    floored at `floor` before the logarithm.  from_matrix: any non-negative [n, 201] matrix, n <= 128."""

    def __init__(self, n_mels=80, f_min=0.0, f_max=8000.0, scale="htk", norm=None, power=2, floor=1e-10):
        W, self.empty_bands = design(n_mels, f_min, f_max, scale, norm)
        self._set(W, power, floor)

    @classmethod
    def from_matrix(cls, W, power=2, floor=1e-10):
        self = cls.__new__(cls)
        W = np.array(W, dtype=np.float64)
        if W.ndim != 2 or W.shape[1] != spec.BINS:
            raise ValueError("from_matrix: a [n, %d] matrix" % spec.BINS)
        self._set(W, power, floor)
        self.empty_bands = int((~self.matrix32.astype(bool).any(axis=1)).sum())
        return self

    def _set(self, W, power, floor):
        self.matrix = np.ascontiguousarray(W, dtype=np.float64)
        self.n_mels = self.matrix.shape[0]
        self.power, self.floor = int(power), float(floor)
        self._handles = {}

    @property
    def matrix32(self):
        """The stored matrix: float32, what the device multiplies with."""
        with np.errstate(over="ignore"):
            return self.matrix.astype(np.float32)

    def spans(self):
        """(first, count) per band: from its first to its last non-zero float32 weight (count 0: an empty band)."""
        nz = self.matrix32 != 0
        first = np.where(nz.any(axis=1), nz.argmax(axis=1), 0)
        last = np.where(nz.any(axis=1), spec.BINS - 1 - nz[:, ::-1].argmax(axis=1), -1)
        return first.astype(np.int64), (last - first + 1).clip(min=0).astype(np.int64)

    def reference(self, rows):
        """The header's definition in float64 on the float32-rounded matrix: rows [n, 201] (float32 log-magnitudes) ->
        [n, n_mels] float64, ln(max(W32 @ exp(min(power * x, 88)), float32(floor)))."""
        x = np.asarray(rows, dtype=np.float32).astype(np.float64).reshape(-1, spec.BINS)
        p = np.exp(np.minimum(self.power * x, MAX_EXPONENT))
        mel = p @ self.matrix32.astype(np.float64).T
        return np.log(np.maximum(mel, np.float64(np.float32(self.floor))))

    # ---- the device object, one per engine, opened when first used ---------------------------
    def handle(self, engine):
        """The nhans_fbank of this filterbank on `engine`'s context."""
        key = engine.handle.value
        h, ref = self._handles.get(key, (None, None))
        if h is not None and ref() is not engine:       # (a closed engine's context address, taken again by a new one)
            hip.load().nhans_fbank_close(self._handles.pop(key)[0])
            h = None
        if h is None:
            h = ctypes.c_void_p()
            hip.check(hip.load().nhans_fbank_open(engine.handle, self.matrix.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                                  self.n_mels, self.power, self.floor, engine._stream(), ctypes.byref(h)))
            self._handles[key] = (h, weakref.ref(engine))
        return h

    def close(self):
        for h, _ in self._handles.values():
            hip.load().nhans_fbank_close(h)
        self._handles = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
