"""Shared pieces of the whole-tensor layer tests (tests/test_gpu_layers.py on the device, tests/test_oracle.py for the CPU
half): the batch, the float64 / float32 CPU references of all 25 stored tensors, the accuracy bar, the comparison
helper that says WHERE a tensor is wrong, and the faults planted in weights.

The yardstick of the bar is the float32 CPU restatement (oracle/torch_ref.py in float32) against the same code in
float64 -- what any correct float32 implementation of the layer may differ by --, never the device's own output:

    bar(t) = K * max|cpu32 - f64| + F * max|f64|          one (K, F) per arithmetic mode, BAR below

and whatever (K, F) are, bar(t) must stay below CAP * max|f64| (2e-5: a fifth of the sampled block check's 1e-4, a tenth
of what a whole layer's lost `lo` half costs).  profiles/layers/README.md holds the measurement (K, F) come from.
"""
import numpy as np
import torch

import nhans_amd  # noqa: F401
from nhans_amd import apply, spec, synth, weights
import oracle.nhans_oracle as O
from oracle.torch_ref import TorchRef
import weight_recipes as R

# ---- the batch ---------------------------------------------------------------------------------------------------
# Three clips in one call: a clip edge after frame 10, a one-frame clip (frame 11: its window is 34 rows of padding),
# another edge, nine frames.  21 frames x pixels per frame is a multiple of no tile size of the conv kernels, so the last
# tile of every launch is ragged and tiles straddle frame windows and clips:
#   resblock1 (7035 px/frame): 147735 = 23 mod 128, 23 mod 256, 279 mod 512
#   resblock2 (1818):           38178 = 34 mod 128, 34 mod 256, 290 mod 512
#   resblock3 ( 459):            9639 = 39 mod 128, 167 mod 256, 423 mod 512
#   resblock4 ( 130):            2730 = 42 mod 128, 170 mod 256, 170 mod 512
# (check_batch_geometry() asserts these, and the same for the chunks of fetch (b).)
FRAMES = (11, 1, 9)
FOFF = [0, 11, 12, 21]
TOTAL = 21
# fetch (b): 8 frame windows per pass -- passes [0, 8), [8, 16), [16, 21): a chunk boundary inside clip 0 and one inside
# clip 2; 8 and 5 frames x pixels per frame are multiples of none of 128 / 256 / 512 either
CHUNK = 8
TILES = (128, 256, 512)
N_CTX = 3

GEO = spec.activation_geometry()
NAMES = (["tower %s %s" % (g["name"], k) for g in spec.tower_geometry() for k in ("conv1", "output")]
         + ["stack %s %s" % (g["name"], k) for g in spec.main_geometry() for k in ("conv1", "output")] + ["last_conv"])
TOWER_IDX = list(range(8))
STACK_IDX = list(range(8, 25))

WEIGHTS = {
    "synthetic7": lambda kind: weights.synthetic_weights(kind, 7),
    "heavy": R.heavy,
    "trained_bn": R.trained_bn,
}
# weight sets reference() knows besides those the layer tests run over
OTHER_WEIGHTS = {"one_channel_loud": R.one_channel_loud}

# ---- the bar -----------------------------------------------------------------------------------------------------
CAP = 2e-5
# (K, F) per arithmetic mode, from the measurement on the MI355X in profiles/layers/README.md.  K = 4 was fixed before the
# first run.  A multiple of err_cpu32 alone cannot serve: the worst measured ratio is 5.95 (f32, tensor 6, `trained_bn`), twice
# that is 12, and 12 x err_cpu32 exceeds the cap on the tensors whose float32 level is above 1.7e-6 of max.  So F carries
# what K = 4 leaves -- 1.18e-6 of max in f32, 0.87e-6 in f16x3 at the worst tensor -- doubled.  The largest bar this gives on
# any tensor of the suite is 1.03e-5 of max, half the cap.  (What F stands for: the kernels of both modes add a conv's
# 2,048 .. 8,192 products in one fixed order into f32 accumulators and multiply by BatchNorm scales folded into f32 weights;
# the CPU's float32 convs add in blocks.  The two modes and all conv variants differ from float64 by the same 4.5e-6 of max
# on the worst tensor, the tower's last: it is the order of the additions, not a kernel.)
BAR = {"f32": (4.0, 2.4e-6), "f16x3": (4.0, 1.8e-6)}
LOGIT_TOL = 1e-4        # the existing bars of the averaged outputs (tests/test_gpu_recipes.py)
EMB_TOL = 2e-5


def check_batch_geometry():
    px = sorted({GEO[i]["hout"] * GEO[i]["wout"] for i in STACK_IDX[:-1]}, reverse=True)
    assert px == [7035, 1818, 459, 130], px
    chunks = [TOTAL] + [min(CHUNK, TOTAL - g0) for g0 in range(0, TOTAL, CHUNK)]
    for n in chunks:
        for p in px:
            for t in TILES:
                assert (n * p) % t, (n, p, t)
    # a chunk boundary of fetch (b) strictly inside a clip
    assert any(FOFF[i] < g0 < FOFF[i + 1] for g0 in range(CHUNK, TOTAL, CHUNK) for i in range(len(FRAMES)))


def features():
    """Three short mixtures (FRAMES) and three 200-frame contexts -- noise, silence (the constant ln 1e-5: every border
    tap of the strided 8x4 convs reads zero padding against a large constant), a speaker -- as the oracle computes them,
    rounded to float32: what the C ABI takes, and what both CPU references continue from."""
    lms = []
    for i, nfr in enumerate(FRAMES):
        mix = apply.trim_to_frames(apply.normalise(synth.mixture(61 + i, (400 + (nfr - 1) * 160) / 16000.0)))
        lm = O.logmag_phase(O.stft(mix))[0].astype(np.float32)
        assert lm.shape[0] == nfr, lm.shape
        lms.append(lm)
    ctx = np.stack([O.context(O.logmag_phase(O.stft(apply.normalise(w)))[0])
                    for w in (synth.noise_context(61), synth.silent(), synth.speaker_context(62))])
    assert np.all(ctx[1] == np.log(1e-5))
    return lms, ctx.astype(np.float32)


def clip_embeddings(emb):
    """Clip i is conditioned on (context i, context i + 1): one (a, b) row pair per clip."""
    n = len(FRAMES)
    return emb[[i % N_CTX for i in range(n)]], emb[[(i + 1) % N_CTX for i in range(n)]]


class Taps:
    """acts: {index: torch tensor NHWC} for all 25 tensors; emb [3,512]; logits and denoised [21,201] -- of one dtype."""


def cpu_taps(W, kind, dtype, lms, ctx, emb_in=None, want=("tower", "stack"), store=None):
    """All stored tensors by oracle/torch_ref.py in `dtype`.  The stack is fed emb_in ([3,512] float32; None: this run's own
    embeddings rounded to float32) so that stack errors are not the tower's.  store: TorchRef's storage hook."""
    ref = TorchRef(W, kind, dtype, store=store)
    t = Taps()
    t.acts, t.emb, t.logits, t.denoised = {}, None, None, None
    with torch.no_grad():
        if "tower" in want:
            t.emb = ref.tower(torch.from_numpy(ctx).to(dtype), t.acts)
        if "stack" in want:
            if emb_in is None:
                emb_in = t.emb.to(torch.float32).numpy()
            ea, eb = clip_embeddings(torch.from_numpy(np.asarray(emb_in, dtype=np.float32)).to(dtype))
            per_clip, outs, dens = [], [], []
            for i, lm in enumerate(lms):
                a = {}
                win = ref.windows(torch.from_numpy(lm).to(dtype))
                o, d = ref.mask_net(win, ea[i][None].expand(len(lm), -1), eb[i][None].expand(len(lm), -1), a)
                per_clip.append(a)
                outs.append(o)
                dens.append(d)
            for idx in STACK_IDX:
                t.acts[idx] = torch.cat([a[idx] for a in per_clip])
            t.logits = torch.cat(outs)
            t.denoised = torch.cat(dens)
    return t


_last_reference = [None, None]


def reference(kind, recipe):
    """(f64 taps, f32 taps, features) of one model and weight set; the last one asked for is kept (0.9 GB)."""
    if _last_reference[0] != (kind, recipe):
        _last_reference[:] = [None, None]
        W = (WEIGHTS.get(recipe) or OTHER_WEIGHTS[recipe])(kind)
        lms, ctx = features()
        t64 = cpu_taps(W, kind, torch.float64, lms, ctx)
        emb_in = t64.emb.to(torch.float32).numpy()
        t32 = cpu_taps(W, kind, torch.float32, lms, ctx, emb_in)
        _last_reference[:] = [(kind, recipe), (W, lms, ctx, emb_in, t64, t32)]
    return _last_reference[1]


# ---- the comparison ----------------------------------------------------------------------------------------------
class Verdict:
    def __init__(self, **kw):
        self.__dict__.update(kw)

    def row(self):
        name = getattr(self, "name", None) or NAMES[self.idx]
        return "%2d %-34s %-12s err_hip %.3e  err_cpu32 %.3e  max %.3e  hip/cpu32 %6.2f  hip/max %.2e  bar/max %.2e %s" % (
            self.idx, name, self.mode, self.err_hip, self.err_cpu32, self.m,
            self.err_hip / max(self.err_cpu32, 1e-300), self.err_hip / self.m, self.bar / self.m, "" if self.ok else "FAIL")


def _where(idx, n, h, w, shape, pixel_in_launch, launch_pixels):
    N, H, W_, C = shape
    tags = []
    if h == 0: tags.append("first row")
    if h == H - 1: tags.append("last row")
    if w == 0: tags.append("first column")
    if w == W_ - 1: tags.append("last column")
    for t in TILES:
        if pixel_in_launch >= (launch_pixels // t) * t:
            tags.append("last partial %d-pixel tile of the launch" % t)
    if idx >= 8:
        for i in range(len(FRAMES)):
            if n == FOFF[i]: tags.append("first frame of clip %d" % i)
            if n == FOFF[i + 1] - 1: tags.append("last frame of clip %d" % i)
    return ", ".join(tags) or "interior"


def check_tensor(idx, hip, t64, t32, mode, label=""):
    """hip: the device's tensor `idx` (f32 NHWC, all frames / images of the batch in one array) against the float64 taps,
    ALL elements.  Returns a Verdict: ok, the figures, the worst element's location, per-channel / per-column error maxima
    and a message that names them."""
    K, F = BAR[mode]
    ref = t64.acts[idx]
    hip = hip.detach().cpu()
    assert tuple(hip.shape) == tuple(ref.shape), (idx, hip.shape, ref.shape)
    shape = tuple(ref.shape)
    N, H, W_, C = shape
    d = (hip.to(torch.float64) - ref).abs_()
    err_cpu32 = float((t32.acts[idx].to(torch.float64) - ref).abs_().max())
    m = float(ref.abs().max())
    err_hip = float(d.max()) if bool(torch.isfinite(hip).all()) else float("inf")
    bar = K * err_cpu32 + F * m
    chan = d.amax(dim=(0, 1, 2))
    col = d.amax(dim=(0, 1, 3))
    flat = int(d.argmax())
    n, r = divmod(flat, H * W_ * C)
    h, r = divmod(r, W_ * C)
    w, c = divmod(r, C)
    neg = float(hip.min())
    problems = []
    if not err_hip <= bar:
        problems.append("max|hip - f64| %.3e above the bar %.3e (= %g x err_cpu32 %.3e + %g x max %.3e)" % (err_hip, bar, K, err_cpu32, F, m))
    if not bar < CAP * m:
        problems.append("the bar %.3e is not below the cap %g x max = %.3e (err_cpu32 %.3e)" % (bar, CAP, CAP * m, err_cpu32))
    if not err_cpu32 <= CAP * m:
        problems.append("float32 CPU against float64 %.3e above %g x max: the yardstick itself is off" % (err_cpu32, CAP))
    if not neg >= 0.0:
        problems.append("a post-ReLU tensor holds %.3e" % neg)       # (zeros of the references: |hip| is its error, under the bar above)
    over = torch.nonzero(chan > bar).flatten().tolist()
    v = Verdict(idx=idx, mode=mode, ok=not problems, err_hip=err_hip, err_cpu32=err_cpu32, m=m, bar=bar, worst=(n, h, w, c),
                chan_err=chan, col_err=col, channels_over=over, message="")
    if problems:
        topc = torch.topk(chan, min(5, C))
        topw = torch.topk(col, min(5, W_))
        v.message = ("tensor %d (%s) %s %s: %s; worst element (%s %d, h %d, w %d, c %d) of %s: hip %.9g f64 %.9g cpu32 %.9g [%s]; "
                     "%d of %d channels above the bar; channel maxima %s; column maxima %s" % (
                         idx, NAMES[idx], mode, label, "; ".join(problems), "frame" if idx >= 8 else "image", n, h, w, c, shape,
                         float(hip[n, h, w, c]), float(ref[n, h, w, c]), float(t32.acts[idx][n, h, w, c]),
                         _where(idx, n, h, w, shape, n * H * W_ + h * W_ + w, N * H * W_), len(over), C,
                         ", ".join("c%d %.2e" % (int(i), float(e)) for e, i in zip(topc.values, topc.indices)),
                         ", ".join("w%d %.2e" % (int(i), float(e)) for e, i in zip(topw.values, topw.indices))))
    return v


# ---- the three arrays a caller receives: same bar, same verdict, same table ------------------------------------------
# (numbered after the 25 stored tensors in the table of rows)
HEADS = {"embeddings": (25, "head embeddings [n,512]"), "logits": (26, "head logits [T,201]"),
         "denoised": (27, "head denoised [T,201]")}


def _where_row(name, r, rows, foff, chunk):
    if name == "embeddings":
        tags = [t for t, hit in (("first image", r == 0), ("last image", r == rows - 1)) if hit]
        if chunk and r % chunk == 0: tags.append("first image of a pass of %d" % chunk)
        return ", ".join(tags) or "interior"
    tags = []
    for i in range(len(foff) - 1):
        if foff[i] <= r < foff[i + 1]:
            tags.append("clip %d" % i)
            if r == foff[i]: tags.append("first frame of clip %d" % i)
            if r == foff[i + 1] - 1: tags.append("last frame of clip %d" % i)
    if r == rows - 1 or (chunk and r % chunk == chunk - 1):
        tags.append("last row of a pass")
    for t in TILES:
        if r >= (rows // t) * t:
            tags.append("last partial %d-row tile of the launch" % t)
    return ", ".join(tags)


def check_head(name, hip, ref64, cpu32, mode, label="", foff=None, chunk=0):
    """One of the arrays a caller receives -- name: "embeddings" [n,512], "logits" or "denoised" [T,201] -- against float64,
    ALL elements, at check_tensor's bar: K x max|cpu32 - f64| + F x max|f64|, (K, F) = BAR[mode], below CAP x max|f64|.
    hip: the device's array; ref64 / cpu32: the float64 reference and its float32 CPU restatement (the yardstick).
    foff: frame offsets of the clips (default: the layer tests' batch when the row count is its 21, else one clip);
    chunk: rows per pass, for the message.  Returns a Verdict like check_tensor's: worst = (row, column), col_err per
    embedding channel / bin, channels_over = the channels / bins above the bar."""
    K, F = BAR[mode]
    idx, title = HEADS[name]
    unit_r, unit_c = ("image", "channel") if name == "embeddings" else ("frame", "bin")
    ref = torch.as_tensor(ref64).to(torch.float64)
    c32 = torch.as_tensor(cpu32)
    hip = torch.as_tensor(hip).detach().cpu()
    assert hip.ndim == 2 and tuple(hip.shape) == tuple(ref.shape) == tuple(c32.shape), (name, hip.shape, ref.shape, c32.shape)
    assert c32.dtype == torch.float32 and hip.dtype in (torch.float32, torch.float64), (c32.dtype, hip.dtype)
    rows, cols = ref.shape
    if foff is None:
        foff = FOFF if (name != "embeddings" and rows == TOTAL) else [0, rows]
    d = (hip.to(torch.float64) - ref).abs_()
    err_cpu32 = float((c32.to(torch.float64) - ref).abs_().max())
    m = float(ref.abs().max())
    err_hip = float(d.max()) if bool(torch.isfinite(hip).all()) else float("inf")
    bar = K * err_cpu32 + F * m
    col = d.amax(dim=0)
    row = d.amax(dim=1)
    r, c = divmod(int(d.argmax()), cols)
    problems = []
    if not err_hip <= bar:
        problems.append("max|hip - f64| %.3e above the bar %.3e (= %g x err_cpu32 %.3e + %g x max %.3e)" % (err_hip, bar, K, err_cpu32, F, m))
    if not bar < CAP * m:
        problems.append("the bar %.3e is not below the cap %g x max = %.3e (err_cpu32 %.3e)" % (bar, CAP, CAP * m, err_cpu32))
    if not err_cpu32 <= CAP * m:
        problems.append("float32 CPU against float64 %.3e above %g x max: the yardstick itself is off" % (err_cpu32, CAP))
    if name == "embeddings" and not float(hip.min()) >= 0.0:
        problems.append("a mean of a post-ReLU tensor is %.3e" % float(hip.min()))
    over = torch.nonzero(col > bar).flatten().tolist()
    v = Verdict(idx=idx, name=title, mode=mode, ok=not problems, err_hip=err_hip, err_cpu32=err_cpu32, m=m, bar=bar, worst=(r, c),
                col_err=col, row_err=row, chan_err=col, channels_over=over, message="")
    if problems:
        topc = torch.topk(col, min(5, cols))
        topr = torch.topk(row, min(5, rows))
        v.message = ("%s %s %s: %s; worst element (%s %d, %s %d) of %s: hip %.9g f64 %.9g cpu32 %.9g [%s]; %d of %d %ss above the "
                     "bar%s; %s maxima %s; %s maxima %s" % (
                         title, mode, label, "; ".join(problems), unit_r, r, unit_c, c, (rows, cols), float(hip[r, c]), float(ref[r, c]),
                         float(c32[r, c]), _where_row(name, r, rows, foff, chunk), len(over), cols, unit_c,
                         (": " + ", ".join("%s %d" % (unit_c, i) for i in over[:8]) + (" ..." if len(over) > 8 else "")) if over else "",
                         unit_c, ", ".join("%s%d %.2e" % (unit_c[0], int(i), float(e)) for e, i in zip(topc.values, topc.indices)),
                         unit_r, ", ".join("%s%d %.2e" % (unit_r[0], int(i), float(e)) for e, i in zip(topr.values, topr.indices))))
    return v


def dead_channels(W, idx):
    """Channels of tensor idx whose BatchNorm has gamma == 0 (tests/weight_recipes.py: trained_bn): relu(beta) everywhere."""
    if idx == 24:
        scope = "last_conv"
    else:
        g = (spec.tower_geometry() + spec.main_geometry())[idx // 2]
        scope = ("embedding/" if idx < 8 else "") + g["name"] + ("_addition" if idx % 2 else "_conv1")
    return np.nonzero(W[scope + "/gamma"].reshape(-1) == 0)[0], W[scope + "/beta"].reshape(-1)


# ---- faults planted in the weights handed to the library ---------------------------------------------------------
def r16(a):
    return a.astype(np.float16).astype(np.float32)


# name: (weight, slice rounded to f16 -- for the arithmetic, a kernel that lost the `lo` half there --, tensor it shows
# in first, the one output channel it touches or None for all)
FAULTS = {
    "out_channel_resblock2_2_conv2": ("resblock2_2_conv2/w", np.s_[:, :, :, 5:6], 15, 5),
    "tap_32_inputs_resblock4_1_conv1": ("resblock4_1_conv1/w", np.s_[1:2, 2:3, 112:144, :], 20, None),
    "kernel_column_resblock1_2_conv1": ("resblock1_2_conv1/w", np.s_[:, 3:4, :, :], 10, None),
    "out_channel_tower_resblock2_1_conv2": ("embedding/noise_resblock2_1_conv2/w", np.s_[:, :, :, 2:3], 3, 2),
}
FAULT_KIND, FAULT_RECIPE = "denoiser", "synthetic7"


def plant(W, fault):
    name, sl, _, _ = FAULTS[fault]
    Wm = dict(W)
    w = W[name].copy()
    w[sl] = r16(w[sl])
    assert (w != W[name]).any()
    Wm[name] = w
    return Wm


def fault_cpu_figures(fault):
    """float64 on the CPU, true weights against planted ones on the layer tests' batch: what the slice does to its own
    tensor (share of the tensor's max, and per channel), to the tensors before it (nothing) and to the averaged output
    today's suite looks at (logits for the stack, embeddings for the tower; absolute)."""
    W, lms, ctx, emb_in, t64, t32 = reference(FAULT_KIND, FAULT_RECIPE)
    name, sl, idx, chan = FAULTS[fault]
    part = "tower" if idx < 8 else "stack"
    f64 = cpu_taps(plant(W, fault), FAULT_KIND, torch.float64, lms, ctx, emb_in, want=(part,))
    m = float(t64.acts[idx].abs().max())
    d = (f64.acts[idx] - t64.acts[idx]).abs()
    before = max(float((f64.acts[i] - t64.acts[i]).abs().max()) for i in (TOWER_IDX if idx < 8 else STACK_IDX) if i < idx)
    out = float((f64.emb - t64.emb).abs().max()) if idx < 8 else float((f64.logits - t64.logits).abs().max())
    return dict(idx=idx, m=m, own=float(d.max()), own_by_channel=d.amax(dim=(0, 1, 2)), before=before, averaged=out,
                err_cpu32=float((t32.acts[idx].to(torch.float64) - t64.acts[idx]).abs().max()))
