"""Shared pieces of the phase-refinement tests (tests/test_gpu_phase.py on the device, tests/test_phase_host.py for the CPU
half): the classes of (log-magnitude, state) inputs, the float64 definition (nhans_amd.phase), the float32 CPU restatement
of one projection and of the free-running iteration, the bar, a comparison that says WHERE a result is wrong -- (class,
frame, bin) -- and the faults planted in the restatement to show that the comparison catches what it is for.

The yardstick of every bar is the float32 CPU restatement against float64 -- what any correct float32 implementation may
differ by --, never the device's own output (the convention of tests/stft_checks.py).

One projection d = P(lm, t), per FRAME f, both sides on the same float32 lm and complex64 t:

    err(f) = max_k |d - d64|        scale(f) = max exp(lm) over frames f - 2 ... f + 2 of the clip
    bar(f) = K * ratio(class) * scale(f) + A

ratio(class) is the restatement's largest err(f) / scale(f) over the frames of the class.  scale reaches two frames either
side because that is how far a frame's samples reach: a quiet frame between loud ones holds their rounding.  The cap -- a
condition, not a measurement -- is K * ratio < 1e-5.  The restatement uses torch rfft / irfft and float32 exp, windows and
sums; measured on the CPU its ratio is 0.6 - 1.5e-7 on every class here, 15 x under the cap.

Free-running (N iterations, the state fed back): inc[n] is held to K times the restatement's largest relative difference
from float64 over the N iterations, the final waveform to K times the restatement's largest sample difference.  Where the
restatement itself is further than 1e-3 of the figure from float64 the iteration is ill-conditioned there (the phases of
near-zero bins) and only the teacher-forced check -- the float64 state, rounded, fed to one projection -- speaks.
"""
import os

import numpy as np
import torch

import nhans_amd  # noqa: F401
from nhans_amd import phase

WIN, HOP, BINS = phase.WIN, phase.HOP, phase.BINS
RUN = 20                                    # frames per run of the projection kernel (kPhaseRun)
FLOOR = float(np.log(1e-5))
K = 4.0                                     # tests/stft_checks.py's K
A = 1e-10
CAP = 1e-5
ILL = 1e-3                                  # free-running: the restatement's own relative difference above which it is no yardstick
COUNTS = (1, 2, 3, 4, 5, RUN - 1, RUN, RUN + 1, 2 * RUN + 1)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class Verdict:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def unit_state(ph):
    """cos + i sin of float32 phases as complex64: a unit-modulus state."""
    ph = np.asarray(ph, dtype=np.float32)
    return (np.cos(ph.astype(np.float64)) + 1j * np.sin(ph.astype(np.float64))).astype(np.complex64)


def demo_rows(name="example2"):
    """(lm, ph, target, mixed): the clean target's log-magnitudes with the mixture's phases, float32 [T, 201], of a demo
    triple of tests/golden/score_demo_pairs.npz -- the ceiling of any mask with mixed phase -- and the two signals."""
    g = np.load(os.path.join(GOLDEN, "score_demo_pairs.npz"))
    tgt, mix = g[name + "_target"], g[name + "_mixed"]
    lm = np.log(np.abs(phase.analyse(tgt)) + 1e-5).astype(np.float32)
    ph = np.angle(phase.analyse(mix)).astype(np.float32)
    return lm, ph, tgt, mix


def uniform_case(t, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(FLOOR, 0.0, (t, BINS)).astype(np.float32), rng.uniform(-np.pi, np.pi, (t, BINS)).astype(np.float32))


def special_state(t=RUN + 1, seed=4107):
    """A state with zero, sub-normal, barely normal and large entries among ordinary ones of any modulus."""
    rng = np.random.default_rng(seed)
    lm, ph = uniform_case(t, seed)
    z = (rng.uniform(0.25, 4.0, (t, BINS)) * np.exp(1j * ph.astype(np.float64))).astype(np.complex64)
    flat = z.reshape(-1)
    idx = rng.permutation(flat.size)
    flat[idx[0:40]] = 0.0
    flat[idx[40:80]] = np.complex64(1e-40 - 3e-41j)             # sub-normal components
    flat[idx[80:120]] = np.complex64(-2e-39 + 1e-39j)           # |z| = 2.2e-39, below the smallest normal 1.18e-38
    flat[idx[120:160]] = np.complex64(3e-30 + 4e-30j)           # normal, its square is not
    flat[idx[160:200]] = np.complex64(-3e30 + 4e30j)
    flat[idx[200:240]] = np.complex64(0.0 - 1e-40j)
    return lm, z


def classes():
    """[(name, lm [T, 201] float32, t [T, 201] complex64)]: fixed seeds."""
    out = []
    for t in COUNTS:
        lm, ph = uniform_case(t, 4000 + t)
        out.append(("uniform T=%d" % t, lm, unit_state(ph)))
    lm, ph, _, _ = demo_rows("example2")
    out.append(("demo magnitudes", lm, unit_state(ph)))
    rng = np.random.default_rng(4101)
    ph30 = rng.uniform(-np.pi, np.pi, (30, BINS)).astype(np.float32)
    alt = np.where((np.arange(30) % 2 == 0)[:, None], np.float32(0.0), np.float32(np.log(1e-4))) * np.ones((1, BINS), np.float32)
    out.append(("loud and quiet frames by 1e-4", alt.astype(np.float32), unit_state(ph30)))
    out.append(("lm in [0, 16]", rng.uniform(0.0, 16.0, (30, BINS)).astype(np.float32), unit_state(ph30)))
    lm, z = special_state()
    out.append(("zero and sub-normal state", lm, z))
    return out


def offsets(counts):
    off = [0]
    for n in counts:
        off.append(off[-1] + int(n))
    return off


# ---- float32 CPU restatement ---------------------------------------------------------------------------------------
# Bins the forward pass writes as conjugates of bins 400 - k of its 20 x 20 transform (tests/stft_checks.py: MIRRORED)
MIRRORED = np.array([b for b in range(BINS) if (WIN - b) // 20 >= 10 and 1 <= (WIN - b) % 20 <= 9 and b > 0])
FAULTS = ("halo_dropped", "nyquist_imag", "conj_dropped")


def _unit32(t):
    t = torch.from_numpy(np.ascontiguousarray(t, dtype=np.complex64))
    m = t.abs().to(torch.float64)                                    # (the modulus of tiny entries does not survive float32)
    small = m < phase.SMALLEST_NORMAL
    u = (t.to(torch.complex128) / torch.where(small, torch.ones_like(m), m)).to(torch.complex64)
    return torch.where(small, torch.ones_like(u), u)


def cpu32_project(lm, t, fault=None):
    """One projection in float32: exp, the product with u(t), torch.fft.irfft, synthesis window, overlap-add, analysis window,
    torch.fft.rfft -> complex64 [T, 201].  fault: one of FAULTS, planted the way the kernel could get it wrong:
    halo_dropped  the second run of the clip (frames RUN ...) overlap-adds without frame RUN - 2, its first halo frame;
    nyquist_imag  frames (2k, 2k + 1) share one complex inverse transform; with the imaginary part of bin 200 kept,
                  Im c_a[200] shows up in frame b and -Im c_b[200] in frame a, as (-1)^n / 400;
    conj_dropped  the mirrored bins of the forward pass are stored without their conjugation."""
    lm = torch.from_numpy(np.ascontiguousarray(lm, dtype=np.float32))
    c = torch.exp(lm) * _unit32(t)
    fr = torch.fft.irfft(c, n=WIN, dim=1)
    assert fr.dtype == torch.float32
    n = fr.shape[0]
    if fault == "nyquist_imag":
        alt = torch.from_numpy(np.where(np.arange(WIN) % 2 == 0, 1.0, -1.0).astype(np.float32)) / np.float32(WIN)
        im = c[:, BINS - 1].imag
        fr = fr.clone()
        for a in range(0, n - 1, 2):
            fr[a + 1] += im[a] * alt
            fr[a] -= im[a + 1] * alt
    fr = fr * torch.from_numpy(phase.synthesis_window().astype(np.float32))[None, :]
    x = torch.zeros((n - 1) * HOP + WIN, dtype=torch.float32)
    for i in range(n):
        x[i * HOP:i * HOP + WIN] += fr[i]
    if fault == "halo_dropped" and n > RUN:
        x[RUN * HOP:(RUN - 2) * HOP + WIN] -= fr[RUN - 2][2 * HOP:]
    idx = torch.arange(WIN)[None, :] + HOP * torch.arange(n)[:, None]
    d = torch.fft.rfft(x[idx] * torch.from_numpy(phase.analysis_window().astype(np.float32))[None, :], n=WIN, dim=1).numpy()
    assert d.dtype == np.complex64
    if fault == "conj_dropped":
        d[:, MIRRORED] = np.conj(d[:, MIRRORED])
    return d


def scale(lm):
    """scale(f): the largest exp(lm) over frames f - 2 ... f + 2 of the clip, float64 [T]."""
    m = np.exp(np.asarray(lm, dtype=np.float64)).max(axis=1)
    n = len(m)
    return np.array([m[max(0, f - 2):min(n, f + 3)].max() for f in range(n)])


def reference64(lm, t):
    return phase.project_reference(np.asarray(lm, dtype=np.float64), np.asarray(t).astype(np.complex128))


_ratios = {}


def yardstick_ratio(key, lm, t):
    """ratio(class) of the module docstring for one clip; kept per key."""
    if key not in _ratios:
        err = np.abs(cpu32_project(lm, t).astype(np.complex128) - reference64(lm, t)).max(axis=1)
        _ratios[key] = float((err / scale(lm)).max())
    return _ratios[key]


def check_project(label, d, lm, t, ratio, ref=None):
    """d (complex64 [T, 201]) as P(lm, t) against the float64 definition, every frame and bin.  Verdict: ok, message, worst =
    (frame, bin) of the largest err / bar, rel = largest err / scale (the device's figure beside `ratio`)."""
    ref = reference64(lm, t) if ref is None else ref
    d = np.asarray(d)
    if d.shape != ref.shape or d.dtype != np.complex64:
        return Verdict(ok=False, message="class %s: %s %s for %s frames x bins" % (label, d.shape, d.dtype, ref.shape), worst=None, rel=np.inf)
    problems = []
    if not K * ratio < CAP:
        problems.append("the bar %g x %.3e is not below the cap %g of the scale" % (K, ratio, CAP))
    e = np.abs(d.astype(np.complex128) - ref)
    e[~np.isfinite(e)] = np.inf
    err, sc = e.max(axis=1), scale(lm)
    bar = K * ratio * sc + A
    f = int(np.argmax(err / bar))
    k = int(e[f].argmax())
    if not err[f] <= bar[f]:
        problems.append("|d - d64| = %.3e above the bar %.3e (= %g x %.3e x scale %.3e + %g) at class %s, frame %d of %d, bin %d: "
                        "%r for %r; %d frames above their bar" % (err[f], bar[f], K, ratio, sc[f], A, label, f, len(err), k,
                                                                  complex(d[f, k]), complex(ref[f, k]), int((err > bar).sum())))
    return Verdict(ok=not problems, message="; ".join(problems), worst=(f, k), rel=float((err / sc).max()), ratio=ratio, label=label)


# ---- free-running --------------------------------------------------------------------------------------------------
def cpu32_reference(lm, ph, iters, alpha=0.0):
    """The iteration in float32: the state complex64, every projection cpu32_project, the momentum step and the final
    synthesis in float32 -> dict(inc [N] float64 of float32 terms, wave float32, phase float32)."""
    lm32 = np.ascontiguousarray(lm, dtype=np.float32)
    t = unit_state(ph)
    a = np.exp(lm32)                                                 # float32
    den = float((a.astype(np.float64) ** 2).sum())
    inc, prev = [], None
    for _ in range(iters):
        d = cpu32_project(lm32, t)
        e = (np.abs(d) - a).astype(np.float32)
        inc.append(float((e.astype(np.float64) ** 2).sum()) / den)
        t = (d + np.float32(alpha) * (d - (d if prev is None else prev))).astype(np.complex64)
        prev = d
    ph_out = np.asarray(ph, dtype=np.float32) if iters == 0 else np.angle(t).astype(np.float32)
    c = torch.polar(torch.exp(torch.from_numpy(lm32)), torch.from_numpy(ph_out))
    fr = torch.fft.irfft(c, n=WIN, dim=1) * torch.from_numpy(phase.synthesis_window().astype(np.float32))[None, :]
    x = torch.zeros((len(lm32) - 1) * HOP + WIN, dtype=torch.float32)
    for i in range(len(lm32)):
        x[i * HOP:i * HOP + WIN] += fr[i]
    return {"inc": np.array(inc), "wave": x.numpy(), "phase": ph_out}


def free_running_yardstick(lm, ph, iters, alpha):
    """-> (float64 reference dict, inc_rel: the restatement's largest |inc32 - inc64| / inc64 over the iterations, wave_abs:
    its largest sample difference, wave_max: the reference waveform's peak)."""
    ref = phase.reference(np.asarray(lm, dtype=np.float64), np.asarray(ph, dtype=np.float32), iters, alpha)
    c32 = cpu32_reference(lm, ph, iters, alpha)
    inc_rel = float((np.abs(c32["inc"] - ref["inc"]) / ref["inc"]).max())
    wave_abs = float(np.abs(c32["wave"].astype(np.float64) - ref["wave"]).max())
    return ref, inc_rel, wave_abs, float(np.abs(ref["wave"]).max())
