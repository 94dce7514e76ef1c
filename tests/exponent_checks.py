"""Shared pieces of the exponent tests (tests/test_gpu_exponents.py on the device, tests/test_exponent_checks_host.py for
the device-free half): every stored tensor of the split-f16 mode is held as hi + lo f16 at a per-tensor power-of-two
exponent, and whether the stored value is right depends on where |x * 2^-e| falls -- above the limit it is clamped and
the sticky STATUS_SATURATED bit must say so, far below it the lo half and then the hi half turn into f16 subnormals.

Everything expected here comes from the float64 reference of tests/layer_checks.py (same batch, same bar), never from
the device:

  * A[j] = max|t64.acts[j]|, r[j] = A[j] * 2^-E[j] for the exponents E READ BACK after they were set (ties change them);
  * expected(): must the status be clean, must it be flagged, or may it be either -- from r of the tensors the fetch
    WRITES (a fetch runs the production launches: the whole tower for any tower tensor, the stack up to the end of the
    block that writes the tensor asked for, all of it for the heads) with 5 % margins that are conditions, not
    measurements;
  * positions of one tie group at a time, all others at the engine's base exponents: `tight` (largest r of the group in
    [3500, 7000): just inside the Winograd-input limit 7168), `between` ([16000, 32000): outside it, inside f16), `over`
    ([2^17, 2^18): clamped) and `raised` (base + k: subnormal halves);
  * the yardstick of `raised` is the CPU's own emulation of the storage format: the float64 network with
    oracle.torch_ref.split_store at the same exponents, fmt_j = max|t_fmt_j - t64_j|; the bar there is bar_j + 4 fmt_j
    (4 = the project's K);  flushed_store -- the same with subnormal halves set to zero -- is the witness that such a
    bar would catch a path that does not honour them.

A `device` here is anything with set_exponents(E) -> E read back, fetch(i) -> (tensor, status) for i in 0 .. 24,
fetch(EMB) -> (embeddings, status), fetch(HEADS) -> ((logits, denoised), status) and take_status(): the engine on the
GPU, an emulation built from the CPU reference in the host half.
"""
import math

import torch

import nhans_amd  # noqa: F401
from nhans_amd import spec
import layer_checks as L
from oracle import torch_ref as TR

SATURATED = 1                       # hip.STATUS_SATURATED
LIMIT_F16, LIMIT_WINO = 65504.0, 7168.0
EMB, HEADS = 25, 26                 # fetches besides the 25 tensors: nhans_embed, nhans_mask_net (logits 26, denoised 27)
CASES = [("denoiser", "synthetic7"), ("denoiser", "trained_bn"), ("separator", "synthetic7")]
POSITIONS = {"tight": 3500.0, "between": 16000.0, "over": 2.0 ** 17}       # the group's largest r in [lo, 2 lo)
KS = (8, 10, 12, 14, 16)
FACTOR = 4.0                        # fmt's multiple in the raised bar: the project's K (layer_checks.BAR)
MODE = "f16x3"
# k of the `raised` position per case: the smallest of KS at which the flush witness is valid on a tower group and a
# stack group (choose_k; tests/test_exponent_checks_host.py asserts it) ...
K_RAISED = {c: 8 for c in CASES}
# ... at the exponents the built-in calibration of nhans_create gives an engine of the case (deterministic; read on the
# MI355X, tests/test_gpu_exponents.py asserts them)
ENGINE_BASE = {
    ("denoiser", "synthetic7"): [-4, -4, -4, -5, -5, -5, -5, -5, -4, -5, -3, -3, -3, -4, -3, -3, -3, -4, -4, -3, -3, -3, -3, -4, -4],
    ("denoiser", "trained_bn"): [-4, -4, -4, -4, -4, -4, -4, -4, -3, -4, -3, -2, -2, -3, -2, -1, -1, -2, -2, -1, -1, -1, -1, -1, -1],
    ("separator", "synthetic7"): [-4, -4, -4, -5, -5, -5, -5, -5, -5, -5, -3, -3, -3, -4, -3, -3, -3, -4, -4, -3, -3, -3, -3, -4, -4],
}


# ---- ties and groups ---------------------------------------------------------------------------------------------
def ties():
    """Pairs of tensors that feed one accumulator and carry one exponent (host_ctx.hip: tie_exponents)."""
    t = [(2 * (b - 1) + 1, 2 * b) for b in range(1, 4)]
    g = spec.main_geometry()
    return t + [(8 + 2 * (b - 1) + 1, 8 + 2 * b) for b in range(1, 8) if g[b]["cin"] != g[b]["cout"]]


def tie(E):
    E = list(E)
    for i, j in ties():
        E[i] = E[j] = max(E[i], E[j])
    return E


def groups():
    """The 25 singletons merged by ties, in tensor order."""
    out = [[i] for i in range(25)]
    for i, j in ties():
        gi = next(g for g in out if i in g)
        gj = next(g for g in out if j in g)
        if gi is not gj:
            gi += gj
            out.remove(gj)
    return [sorted(g) for g in sorted(out)]


def network(i):
    return L.TOWER_IDX if (i < 8 or i == EMB) else L.STACK_IDX


def written(i):
    """Tensors the fetch of i writes."""
    if i < 8 or i == EMB:
        return list(L.TOWER_IDX)
    if i >= 24:
        return list(L.STACK_IDX)
    return list(range(8, 8 + 2 * ((i - 8) // 2) + 2))


def reader(group):
    """The next stored tensor of the same network, or None."""
    j = max(group) + 1
    return j if j in network(group[0]) else None


def head_of(group):
    return EMB if group[0] < 8 else HEADS


def quiet_before(group):
    """The last tensor before the group whose fetch does not run the group's writer (None: every fetch does -- the whole
    tower runs for any tower tensor, block 0 of the stack for tensors 8 and 9)."""
    i = group[0]
    if i < 8:
        return None
    j = 8 + 2 * ((i - 8) // 2) - 1
    return j if j >= 8 else None


# ---- what the status must be -------------------------------------------------------------------------------------
def verdict_of(r, winograd):
    """r: the stored maxima A * 2^-E of the tensors a fetch writes -> "clean" | "flagged" | "either"."""
    r = list(r)
    if any(x > 1.05 * LIMIT_F16 for x in r):
        return "flagged"
    if all(x < 0.95 * (LIMIT_WINO if winograd else LIMIT_F16) for x in r):
        return "clean"
    return "either"


def position_exponent(amax, position):
    """e with amax * 2^-e in [lo, 2 lo)."""
    return math.floor(math.log2(amax / POSITIONS[position]))


# ---- the yardstick of one case -----------------------------------------------------------------------------------
class Yard:
    """The float64 reference of one (kind, recipe) with the figures of layer_checks.check_tensor / check_head per tensor
    -- err_cpu32, max, bar -- computed once, and the comparison itself on `device` (the tensors of the big layers have
    9.4 M elements; on the GPU a comparison costs nothing beside the launches)."""

    def __init__(self, kind, recipe, device="cpu"):
        self.kind, self.recipe, self.device = kind, recipe, device
        self.W, self.lms, self.ctx, self.emb_in, self.t64, self.t32 = L.reference(kind, recipe)
        t64, t32 = self.t64, self.t32
        r64 = dict(t64.acts)
        r32 = dict(t32.acts)
        r64.update({25: t64.emb, 26: t64.logits, 27: t64.denoised})
        r32.update({25: t32.emb, 26: t32.logits, 27: t32.denoised})
        Kb, Fb = L.BAR[MODE]
        self.ref, self.err32, self.m, self.bar = {}, {}, {}, {}
        for i in range(28):
            self.err32[i] = float((r32[i].to(torch.float64) - r64[i]).abs().max())
            self.m[i] = float(r64[i].abs().max())
            self.bar[i] = Kb * self.err32[i] + Fb * self.m[i]
            self.ref[i] = r64[i].to(device)
        self.ref_cpu = r64
        self.A = [self.m[i] for i in range(25)]
        self._fmt = {}

    def name(self, i):
        return L.NAMES[i] if i < 25 else {25: "head embeddings", 26: "head logits", 27: "head denoised"}[i]

    def r(self, E):
        return [self.A[j] * 2.0 ** -E[j] for j in range(25)]

    def expected(self, i, E, winograd):
        r = self.r(E)
        return verdict_of([r[j] for j in written(i)], winograd)

    def judge(self, i, t, label, extra=0.0, mask=None):
        """Tensor i (25 .. 27: a head) of the device against float64, all elements (mask: those elements only), at
        layer_checks' bar plus `extra`.  -> dict(ok, err, bar, message): the conditions of check_tensor / check_head."""
        t = torch.as_tensor(t).detach().to(self.device)
        ref = self.ref[i]
        assert tuple(t.shape) == tuple(ref.shape), (i, t.shape, ref.shape)
        d = (t.to(torch.float64) - ref).abs_()
        if mask is not None:
            d = d[mask]
        finite = bool(torch.isfinite(t).all())
        err = (float(d.max()) if d.numel() else 0.0) if finite else float("inf")
        bar, m = self.bar[i] + extra, self.m[i]
        problems = []
        if not err <= bar:
            problems.append("max|hip - f64| %.3e above the bar %.3e (= %.3e%s)" % (err, bar, self.bar[i], " + %.3e for the format" % extra if extra else ""))
        if not bar < L.CAP * m:
            problems.append("the bar %.3e is not below the cap %g x max = %.3e" % (bar, L.CAP, L.CAP * m))
        if not self.err32[i] <= L.CAP * m:
            problems.append("float32 CPU against float64 %.3e above %g x max: the yardstick itself is off" % (self.err32[i], L.CAP))
        if i != 26 and i != 27 and not float(t.min()) >= 0.0:
            problems.append("a post-ReLU tensor holds %.3e" % float(t.min()))
        msg = ""
        if problems:
            msg = "%s %s, %s: tensor %d (%s): %s" % (self.kind, self.recipe, label, i, self.name(i), "; ".join(problems))
            if mask is None and finite:        # where: the existing helpers say it
                tc = t.cpu()
                if i < 25:
                    msg += " || " + L.check_tensor(i, tc, self.t64, self.t32, MODE, label).message
                else:
                    nm = {25: "embeddings", 26: "logits", 27: "denoised"}[i]
                    msg += " || " + L.check_head(nm, tc, self.ref[i].cpu(), {25: self.t32.emb, 26: self.t32.logits, 27: self.t32.denoised}[i], MODE, label).message
        return dict(ok=not problems, err=err, bar=bar, base_bar=self.bar[i], m=m, message=msg)

    # ---- the storage format's own cost ---------------------------------------------------------------------------
    def stored_run(self, E, net, flushed=False):
        """The float64 network `net` ("tower" | "stack") with every tensor stored at E: {index: tensor} incl. 25 .. 27."""
        store = (TR.flushed_store if flushed else TR.split_store)(list(E))
        t = L.cpu_taps(self.W, self.kind, torch.float64, self.lms, self.ctx, self.emb_in, want=(net,), store=store)
        out = dict(t.acts)
        if net == "tower":
            out[25] = t.emb
        else:
            out[26], out[27] = t.logits, t.denoised
        return out

    def fmt(self, E, group):
        """fmt_j = max|t_fmt(E)_j - t64_j| for the group's tensors, their reader and the heads: one CPU pass, kept."""
        key = (tuple(E), tuple(group))
        if key not in self._fmt:
            run = self.stored_run(E, "tower" if group[0] < 8 else "stack")
            self._fmt[key] = {j: float((run[j] - self.ref_cpu[j]).abs().max()) for j in fetch_list(group, flat=True)}
        return self._fmt[key]


def fetch_list(group, flat=False):
    """What a position fetches: the group's tensors, their reader, the heads (flat: 26 and 27 for HEADS)."""
    f = list(group) + ([reader(group)] if reader(group) is not None else []) + [head_of(group)]
    if flat and f[-1] == HEADS:
        f = f[:-1] + [26, 27]
    return f


def raised(base, group, k):
    E = list(base)
    for j in group:
        E[j] = base[j] + k
    return tie(E)


# ---- one position of one group on a device -----------------------------------------------------------------------
def _fetch(dev, yard, i, E, winograd, where, failures, rows, extra=None, factor=FACTOR, sink=None):
    """Fetch i, hold the status to expected() and -- unless flagged where it may be -- the tensor(s) to the bar."""
    t, st = dev.fetch(i)
    exp = yard.expected(i, E, winograd)
    flagged = bool(st & SATURATED)
    if st & ~SATURATED:
        failures.append("%s: fetch of %d left status %d" % (where, i, st))
    if exp == "clean" and flagged:
        failures.append("%s: fetch of tensor %d (%s) raised STATUS_SATURATED where every stored maximum is inside the limit (largest r %.1f)" % (
            where, i, yard.name(min(i, 26)), max(yard.r(E)[j] for j in written(i))))
    if exp == "flagged" and not flagged:
        failures.append("%s: fetch of tensor %d (%s) left status 0 with a stored maximum of %.1f: clamped without the flag" % (
            where, i, yard.name(min(i, 26)), max(yard.r(E)[j] for j in written(i))))
    parts = [(26, t[0]), (27, t[1])] if i == HEADS else [(i, t)]
    for j, x in parts:
        if flagged:
            rows.append("%-60s %2d %-34s %-7s flagged" % (where, j, yard.name(j), exp))
            continue
        f = extra.get(j, 0.0) if extra else 0.0
        v = yard.judge(j, x, where, extra=factor * f)
        rows.append("%-60s %2d %-34s %-7s status 0  err/bar %.3f  err/max %.2e%s" % (
            where, j, yard.name(j), exp, v["err"] / v["bar"], v["err"] / v["m"],
            "  fmt/max %.2e  (err - bar)/fmt %.2f" % (f / v["m"], (v["err"] - v["base_bar"]) / f) if f else ""))
        if sink is not None:
            sink.append(dict(tensor=j, err=v["err"], bar=v["base_bar"], fmt=f, m=v["m"]))
        if not v["ok"]:
            failures.append(v["message"])
    return t, st


def check_position(dev, yard, base, group, position, winograd, label, k=None, factor=FACTOR, sink=None):
    """Sets the group to `position` (all other groups at `base`), fetches and judges.  -> (failures, rows).  The caller
    restores the exponents."""
    failures, rows = [], []
    where = "%s, group %s %s" % (label, group, position if k is None else "raised by %d" % k)
    if position == "raised":
        want = raised(base, group, k)
    else:
        e = position_exponent(max(yard.A[j] for j in group), position)
        want = list(base)
        for j in group:
            want[j] = e
    E = list(dev.set_exponents(want))
    if E != tie(want):
        failures.append("%s: exponents read back %s, tie_exponents gives %s" % (where, E, tie(want)))
        return failures, rows
    if position in ("tight", "between"):
        for i in fetch_list(group):
            _fetch(dev, yard, i, E, winograd, where, failures, rows)
    elif position == "raised":
        extra = yard.fmt(E, group)
        for i in fetch_list(group):
            t, st = _fetch(dev, yard, i, E, winograd, where, failures, rows, extra=extra, factor=factor, sink=sink)
            if st:
                failures.append("%s: fetch of %d left status %d at raised exponents" % (where, i, st))
    else:
        r = yard.r(E)
        q = quiet_before(group)
        if q is not None:                   # whose flag it is: the launches before the group's writer leave none
            _, st = dev.fetch(q)
            rows.append("%-60s %2d %-34s before the group: status %d" % (where, q, yard.name(q), st))
            if st:
                failures.append("%s: fetch of tensor %d (%s), before the group's writer, left status %d" % (where, q, yard.name(q), st))
        first = next(j for j in group if r[j] > 1.05 * LIMIT_F16)
        t, st = dev.fetch(first)
        again = dev.take_status()
        rows.append("%-60s %2d %-34s over (r %.0f): status %d, then %d" % (where, first, yard.name(first), r[first], st, again))
        if not st & SATURATED:
            failures.append("%s: tensor %d (%s) stored with a maximum of %.0f left status %d: clamped without the flag" % (
                where, first, yard.name(first), r[first], st))
        if again:
            failures.append("%s: a second take_status() returned %d: the bit is read-and-clear" % (where, again))
        s = yard.ref[first].abs() * 2.0 ** -E[first]
        t = torch.as_tensor(t).to(yard.device)
        hi = s >= 1.1 * LIMIT_F16
        clamp = LIMIT_F16 * 2.0 ** E[first]
        wrong = int((t[hi].to(torch.float64) != clamp).sum())
        if wrong or not int(hi.sum()):
            failures.append("%s: tensor %d (%s): %d of %d elements beyond 1.1 x 65504 are not 65504 x 2^%d exactly" % (
                where, first, yard.name(first), wrong, int(hi.sum()), E[first]))
        if all(r[j] <= 0.9 * LIMIT_F16 for j in group if j < first):       # (its inputs are whole)
            v = yard.judge(first, t, where + " (elements below 0.9 x 65504)", mask=s <= 0.9 * LIMIT_F16)
            rows.append("%-60s %2d %-34s over: %d clamped elements exact, the unclamped: err/bar %.3f" % (
                where, first, yard.name(first), int(hi.sum()), v["err"] / v["bar"]))
            if not v["ok"]:
                failures.append(v["message"])
    return failures, rows


# ---- an emulated device, from the CPU reference ------------------------------------------------------------------
class Emulated:
    """What a device would hand back if it stored every tensor with `store` (oracle.torch_ref: split_store,
    flushed_store) and raised the flag by `flag` ("right": a stored maximum at or above 65504, the rule of a device with
    the Winograd form off; "never"; "always").  One CPU pass per network and set of exponents."""

    def __init__(self, yard, store=TR.split_store, flag="right"):
        self.yard, self.store, self.flag = yard, store, flag
        self.E, self.runs, self.status = None, {}, 0

    def set_exponents(self, E):
        self.E = tie(E)
        self.runs = {}
        return list(self.E)

    def fetch(self, i):
        net = "tower" if (i < 8 or i == EMB) else "stack"
        if net not in self.runs:
            self.runs[net] = self.yard.stored_run(self.E, net, flushed=self.store is TR.flushed_store)
        run = self.runs[net]
        r = self.yard.r(self.E)
        over = any(r[j] >= LIMIT_F16 for j in written(i))
        if self.flag == "always" or (self.flag == "right" and over):
            self.status |= SATURATED
        t = (run[26].float(), run[27].float()) if i == HEADS else run[i].float()
        return t, self.take_status()

    def take_status(self):
        st, self.status = self.status, 0
        return st


# ---- the choice of k ---------------------------------------------------------------------------------------------
def witness(yard, base, group, k, factor=FACTOR):
    """Is a path that flushes f16 subnormals caught at `group` raised by k?  -> dict(valid, capped, flushed, need, ...)
    for the reader i + 1 of the group: valid iff max|t_flushed - t64| >= 5 x (bar + factor x fmt), capped iff
    bar_j + factor x fmt_j < CAP x max for the group's tensors and the reader."""
    E = raised(base, group, k)
    fmt = yard.fmt(E, group)
    rd = reader(group)
    run = yard.stored_run(E, "tower" if group[0] < 8 else "stack", flushed=True)
    flushed = float((run[rd] - yard.ref_cpu[rd]).abs().max())
    need = 5 * (yard.bar[rd] + factor * fmt[rd])
    capped = all(yard.bar[j] + factor * fmt[j] < L.CAP * yard.m[j] for j in list(group) + [rd])
    return dict(valid=flushed >= need, capped=capped, flushed=flushed, need=need, reader=rd, fmt=fmt, run=run, E=E)


def choose_k(yard, base):
    """The smallest k of KS for which the flush witness is valid (and the cap holds) on at least one tower group and one
    stack group -> (k, tower group, stack group) or None.  Minutes of CPU: run once, the result is K_RAISED."""
    for k in KS:
        found = []
        for net in (L.TOWER_IDX, L.STACK_IDX):
            for g in groups():
                if g[0] in net and reader(g) is not None:
                    w = witness(yard, base, g, k)
                    if w["valid"] and w["capped"]:
                        found.append(g)
                        break
        if len(found) == 2:
            return k, found[0], found[1]
    return None
