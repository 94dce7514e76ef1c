"""Shared pieces of the head tests (tests/test_gpu_heads.py on the device, tests/test_head_checks_host.py for the CPU half):
the code between the last stored tensor and the arrays a caller receives, taken alone.

    tensor 24 [T,1,26,512] --last_dense 13,312 -> 201, + bias--> logits [T,201] --+ centre row--> denoised [T,201]
    tensor  7 [n,23,26,512] --mean over the 598 pixels--> embeddings [n,512]

The tensor is the INPUT here (on the device: its own tap, so nothing before the head is under test and the frame count
is free; on the CPU: the float32 tensor of layer_checks.reference as a stand-in), the reference is one float64 matrix
product or mean of it, the yardstick the same expression in torch float32, the bar layer_checks.check_head's.

Besides the torch float32 yardstick each form is restated in float32 in the order the kernel documents (32 K-groups of
416 for the dense layer, each from a zeroed accumulator, added in order; 4 interleaved partial sums added ((0+1)+2)+3
for the pool): recorded next to the first, and the yardstick a bar falls back on if a correct kernel misses the first.
"""
import numpy as np
import torch

import layer_checks as L

BINS, EMB, KDENSE, KGROUPS = 201, 512, 26 * 512, 32
POOL_PIXELS = 23 * 26

# ---- dense head: frame counts one below / above the 128-, 256- and 512-row tiles ------------------------------------
DENSE_T = (1, 129, 257, 513)
CLIPS_513 = [0, 130, 131, 513]          # the three-clip split: a one-frame clip behind the first 128-row tile


def dense_inputs(T, foff=None, seed=5):
    """(log-magnitudes [T,201], frame offsets, ea, eb [nclips,512]) as the split-K stress test builds them."""
    g = torch.Generator().manual_seed(seed * 1000 + T)
    foff = list(foff or [0, T])
    lm = torch.randn(T, BINS, generator=g) * 2.0 - 4.0
    ea = torch.randn(len(foff) - 1, EMB, generator=g) * 0.1
    eb = torch.randn(len(foff) - 1, EMB, generator=g) * 0.1
    return lm, foff, ea, eb


def dense_refs(x24, W, centre):
    """x24: tensor 24, float32 [T,1,26,512] NHWC (flatten order w*512 + c, oracle/torch_ref.py); centre [T,201] float32.
    -> dict of (logits, denoised) pairs: f64, cpu32 (torch float32), cpu32_grouped (float32, the kernel's 32 K-groups)."""
    x = torch.as_tensor(x24).detach().cpu().to(torch.float32)
    T = x.shape[0]
    x = x.reshape(T, KDENSE)
    centre = torch.as_tensor(centre).detach().cpu().to(torch.float32)
    w = torch.from_numpy(np.ascontiguousarray(W["last_dense/w"], dtype=np.float32)).reshape(KDENSE, BINS)
    b = torch.from_numpy(np.ascontiguousarray(W["last_dense/b"], dtype=np.float32)).reshape(BINS)
    with torch.no_grad():
        lg64 = x.double() @ w.double() + b.double()
        lg32 = x @ w + b
        kg = KDENSE // KGROUPS
        tot = torch.zeros(T, BINS, dtype=torch.float32)
        for g in range(KGROUPS):
            tot = tot + x[:, g * kg:(g + 1) * kg] @ w[g * kg:(g + 1) * kg]
        lg32g = tot + b
    return {"f64": (lg64, centre.double() + lg64), "cpu32": (lg32, centre + lg32), "cpu32_grouped": (lg32g, centre + lg32g)}


# ---- pool head ------------------------------------------------------------------------------------------------------
def pool_contexts(n, seed=5):
    """n context images [n,200,201]: seeded noise; of more than one, the last is the constant ln 1e-5 (silence)."""
    g = torch.Generator().manual_seed(seed * 1000 + n)
    ctx = torch.randn(n, 200, BINS, generator=g) * 2.0 - 4.0
    if n > 1:
        ctx[n - 1] = float(np.float32(np.log(1e-5)))
    return ctx


def pool_refs(x7):
    """x7: tensor 7, float32 [n,23,26,512] NHWC -> dict: f64 mean over the 598 pixels, cpu32 (torch float32 mean),
    cpu32_kernel_order (float32: partial sums of pixels p, p + 4, ... for p = 0..3, ((0+1)+2)+3, / 598)."""
    x = torch.as_tensor(x7).detach().cpu().to(torch.float32)
    n = x.shape[0]
    x = x.reshape(n, -1, EMB)
    hw = x.shape[1]
    a = x.numpy()
    part = np.zeros((4, n, EMB), dtype=np.float32)
    for i in range(hw):
        part[i & 3] += a[:, i, :]
    k = (((part[0] + part[1]) + part[2]) + part[3]) / np.float32(hw)
    return {"f64": x.double().mean(dim=1), "cpu32": x.mean(dim=1), "cpu32_kernel_order": torch.from_numpy(k)}


# ---- canaries around caller-owned output buffers --------------------------------------------------------------------
GUARD = 256
SENTINEL = 0x5AFEC0DE           # as float32 3.5e13: nothing the head writes


def guarded(T, device="cpu"):
    """int32 words: GUARD sentinels, T x 201 output words (sentinels too: a word never written shows), GUARD sentinels."""
    return torch.full((2 * GUARD + T * BINS,), SENTINEL, dtype=torch.int32, device=device)


def payload(buf, T):
    """The [T,201] float32 output region of a guarded buffer (a view: row 0 starts GUARD words in)."""
    return buf[GUARD:GUARD + T * BINS].view(torch.float32).view(T, BINS)


def canary_damage(buf, T):
    """-> list of findings (empty: every sentinel intact and every output word written)."""
    w = buf.detach().cpu()
    assert w.dtype == torch.int32 and w.numel() == 2 * GUARD + T * BINS
    out = []
    for what, lo in (("before row 0", 0), ("after row %d" % (T - 1), GUARD + T * BINS)):
        bad = torch.nonzero(w[lo:lo + GUARD] != SENTINEL).flatten().tolist()
        if bad:
            out.append("%d sentinel words %s overwritten, first at word %d of the guard (0x%08x)" % (
                len(bad), what, bad[0], int(w[lo + bad[0]]) & 0xFFFFFFFF))
    left = torch.nonzero(w[GUARD:GUARD + T * BINS] == SENTINEL).flatten().tolist()
    if left:
        out.append("%d output words never written, first (row %d, bin %d)" % ((len(left),) + divmod(left[0], BINS)))
    return out


# ---- one-hot conditioning -------------------------------------------------------------------------------------------
ONEHOT_FOFF = [0, 1, 2, 3, 4]
ONEHOT_TENSORS = (8, 9, 22, 23)


def onehot_embeddings():
    """Four one-frame clips: zeros / zeros, e0 / zeros, e511 / e256, zeros / e511 -- a one-hot vector picks one row of
    cond.w: the first and last row of each half (and of the kernel's first and last K-slice), and the first row of the
    fourth slice (512 + 256)."""
    ea = np.zeros((4, EMB), dtype=np.float32)
    eb = np.zeros((4, EMB), dtype=np.float32)
    ea[1, 0] = 1.0
    ea[2, 511], eb[2, 256] = 1.0, 1.0
    eb[3, 511] = 1.0
    return ea, eb


def onehot_logmag(seed=5):
    g = torch.Generator().manual_seed(seed * 1000 + 4)
    return (torch.randn(4, BINS, generator=g) * 2.0 - 4.0).numpy().astype(np.float32)


def onehot_taps(W, kind, dtype, embeddings=None):
    """The stack's tensors, logits and denoised rows of the four clips by oracle/torch_ref.py in `dtype`; embeddings:
    (ea, eb) in place of the one-hot ones."""
    from oracle.torch_ref import TorchRef
    lm = onehot_logmag()
    ea, eb = embeddings or onehot_embeddings()
    ref = TorchRef(W, kind, dtype)
    t = L.Taps()
    t.acts, t.emb = {}, None
    with torch.no_grad():
        win = torch.cat([ref.windows(torch.from_numpy(lm[i:i + 1]).to(dtype)) for i in range(4)])
        t.logits, t.denoised = ref.mask_net(win, torch.from_numpy(ea).to(dtype), torch.from_numpy(eb).to(dtype), t.acts)
    return t


# ---- faults planted in last_dense/w ---------------------------------------------------------------------------------
def dense_logits32_in_order(x, W):
    """The dense layer in float32 as ELEMENTWISE operations in the order the kernel documents -- 32 K-groups of 416, each
    summed from zero in ascending k (one rounded product, one rounded addition per term), the groups added in order, then
    the bias: the same bits on every host, whatever its CPU, libraries and thread count.  x [T,13312] float32."""
    xa = np.ascontiguousarray(torch.as_tensor(x).detach().cpu().to(torch.float32).numpy()).reshape(-1, KDENSE)
    w = np.ascontiguousarray(W["last_dense/w"], dtype=np.float32).reshape(KDENSE, BINS)
    kg = KDENSE // KGROUPS
    tot = np.zeros((xa.shape[0], BINS), dtype=np.float32)
    for g in range(KGROUPS):
        acc = np.zeros_like(tot)
        for k in range(g * kg, (g + 1) * kg):
            acc += xa[:, k, None] * w[k]
        tot += acc
    return torch.from_numpy(tot + np.asarray(W["last_dense/b"], dtype=np.float32).reshape(BINS))


# name: (weight, slice rounded to f16, the one bin it touches or None for many).  Each is a witness of what check_head adds:
# in float64 on the layer tests' batch the logits move by at least 5 x check_head's bar AND by less than the LOGIT_TOL bar
# the suite had before (tests/test_head_checks_host.py asserts both).
#   The bar of that statement is the ISOLATED head's (the fault lives in last_dense/w alone, nothing up to tensor 24 moves):
# reference = float64 product of the float64 tensor 24 rounded to float32, yardstick = dense_logits32_in_order of the same
# input -- deterministic, where oracle/torch_ref.py in float32 through the whole stack differs from host to host (its
# convolutions add in an order that follows the CPU and the thread count: 1.9e-6 .. 8.1e-6 on these logits, which moves five
# times the bar from 7.5e-5 to 2.0e-4, past the old bar).  K, F and the cap are layer_checks' own.
#   `separator heavy`: max|logit| 3.14, in-order float32 error 1.46e-6, bar 1.34e-5 (f32 mode), five times it 6.7e-5, old
# bar 1e-4.  Column 200 over all rows moves bin 200 by 1.19e-4; halved once, rows 0:6656: 8.7e-5.  The K tail: 32 rows
# (25*512+480 : 26*512) move the logits by 2.4e-5; doubled to 64, 128, 256 rows bin 153 alone moves by 1.7e-4 (one heavy-tailed
# weight row), every other bin by at most 7.8e-5 -- so the K tail is the last 256 rows of bins 0..152: 7.8e-5, 37 bins above 3e-5.
HEAD_FAULT_KIND, HEAD_FAULT_RECIPE = "separator", "heavy"
HEAD_FAULTS = {
    "k_tail_last_dense": ("last_dense/w", np.s_[26 * 512 - 256:26 * 512, 0:153], None),
    "bin_200_last_dense": ("last_dense/w", np.s_[0:KDENSE // 2, 200:201], 200),
}


def plant_head(W, fault):
    name, sl = HEAD_FAULTS[fault][:2]
    Wm = dict(W)
    w = W[name].copy()
    w[sl] = L.r16(w[sl])
    assert (w != W[name]).any()
    Wm[name] = w
    return Wm


_fault_yardstick = {}


def head_fault_cpu_figures(fault):
    """float64 on the CPU, true weights against planted ones on the layer tests' batch.  Only last_dense/w differs (every
    other array of the planted set is the true set's own object), so nothing up to tensor 24 moves and the logits are
    one matrix product of the reference's tensor 24 away.  err_cpu32 / m: the isolated head's deterministic yardstick
    (above); old_bar: LOGIT_TOL's, on the whole-stack float64 logits."""
    W, lms, ctx, emb_in, t64, t32 = L.reference(HEAD_FAULT_KIND, HEAD_FAULT_RECIPE)
    Wm = plant_head(W, fault)
    name = HEAD_FAULTS[fault][0]
    changed = [k for k in W if Wm[k] is not W[k]]
    x = t64.acts[24].reshape(L.TOTAL, KDENSE)
    w64 = torch.from_numpy(W[name]).double().reshape(KDENSE, BINS)
    b64 = torch.from_numpy(W["last_dense/b"]).double().reshape(BINS)
    assert float((x @ w64 + b64 - t64.logits).abs().max()) <= 1e-12 * float(t64.logits.abs().max())
    d = (x @ (torch.from_numpy(Wm[name]).double().reshape(KDENSE, BINS) - w64)).abs()
    if not _fault_yardstick:
        x32 = x.to(torch.float32)
        iso64 = x32.double() @ w64 + b64
        _fault_yardstick.update(m=float(iso64.abs().max()),
                                err=float((dense_logits32_in_order(x32, W).double() - iso64).abs().max()))
    return dict(changed=changed, m=_fault_yardstick["m"], moved=float(d.max()), moved_by_bin=d.amax(dim=0),
                err_cpu32=_fault_yardstick["err"], old_bar=L.LOGIT_TOL * max(1.0, float(t64.logits.abs().max()) / 5.0))
