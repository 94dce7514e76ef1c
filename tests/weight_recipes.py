"""Weight sets for the parity tests beyond `weights.synthetic_weights(kind, 7)` (tests/test_gpu_recipes.py).

The trained checkpoint of the reference is a git-LFS pointer in the tree, so every golden vector and fuzz batch uses
seeded synthetic weights; what the split-f16 arithmetic of the HIP path depends on -- the hi/lo split of weights whose
columns were scaled by a power of two, the Winograd re-split of transformed activations, the activation exponents --
depends on the weight DISTRIBUTION.  These recipes span what a trained or a freshly initialised network looks like:

  seed        the standard recipe with another seed
  heavy       Student-t (3 degrees of freedom) conv / dense weights whose input channels carry a log-uniform scale
              over three decades -- 10^3 of dynamic range inside every weight column --, per-tensor RMS as in the
              standard recipe so that activations stay O(1)
  trained_bn  BatchNorm statistics of a trained net: pop_variance log-uniform 1e-6 .. 10 (BN scale gamma/sqrt(var+1e-3)
              up to 31 gamma, SN/blocks.py:104-108), the convolution in front of each BN scaled per channel by
              sqrt(pop_variance) and pop_mean likewise (in a trained net the statistics ARE those of the activations),
              gamma with 10 % exact zeros (dead channels), beta uniform in [-3, 3]
  tf_init     the reference's own initialisers (SN/main.py:136,142,146,238; SN/blocks.py): truncated normal sigma =
              0.01 for conv / dense weights, sigma = 0 for `*_dense3`, `*_emb` and `last_dense`, zero biases, BatchNorm
              at its TF defaults (gamma 1, beta 0, pop_mean 0, pop_variance 1): `out` is exactly 0 and `denoised` is
              exactly the centre frame of the window.

Beside them, for the calibration tests (tests/calibration_checks.py) and not among RECIPES:

  one_channel_loud  `synthetic7` with one output channel of each of the 25 stored tensors 2^5 times louder and its readers
              compensated: the maximum of every tensor sits in channel 0, 31, 32 or C - 1 in turn.
"""
import zlib

import numpy as np

import nhans_amd  # noqa: F401
from nhans_amd import spec, weights


def _rng(seed, name):
    return np.random.default_rng([int(seed), zlib.crc32(name.encode("utf-8")), 77])


def seed(kind, s):
    return weights.synthetic_weights(kind, s)


def heavy(kind, s=31):
    W = dict(weights.synthetic_weights(kind, s))
    for name, a in W.items():
        scope, leaf = name.rsplit("/", 1)
        if leaf != "w" or a.ndim not in (2, 4) or a.shape[-2] < 16:
            continue                                     # (the one-channel convs and the position MLPs keep their recipe)
        r = _rng(s, name)
        rms = float(np.sqrt(np.mean(a.astype(np.float64) ** 2)))
        t = r.standard_t(3, size=a.shape)
        cin_scale = 10.0 ** r.uniform(-1.5, 1.5, size=a.shape[-2])
        t = t * cin_scale.reshape((1,) * (a.ndim - 2) + (-1, 1))
        t *= rms / np.sqrt(np.mean(t ** 2))
        W[name] = t.astype(np.float32)
    return W


def trained_bn(kind, s=41):
    W = dict(weights.synthetic_weights(kind, s))
    for name in list(W):
        scope, leaf = name.rsplit("/", 1)
        if leaf != "pop_variance":
            continue
        r = _rng(s, name)
        n = W[name].size
        shape = W[name].shape
        old_var = W[name].astype(np.float64).reshape(-1)
        addition = scope.endswith("_addition")
        # the `_addition` BatchNorm sees conv2 + shortcut: its statistics follow two producers, keep them within a decade
        var = 10.0 ** (r.uniform(-1.0, 1.0, n) if addition else r.uniform(-6.0, 1.0, n))
        gain = np.sqrt((var + spec.BN_EPS) / (old_var + spec.BN_EPS))          # BN scale changes by 1 / gain ...
        W[name] = var.reshape(shape).astype(np.float32)
        W[scope + "/pop_mean"] = (W[scope + "/pop_mean"].astype(np.float64).reshape(-1) * gain).reshape(shape).astype(np.float32)
        gamma = W[scope + "/gamma"].astype(np.float64).reshape(-1).copy()
        gamma[r.random(n) < 0.10] = 0.0
        W[scope + "/gamma"] = gamma.reshape(shape).astype(np.float32)
        W[scope + "/beta"] = r.uniform(-3.0, 3.0, n).reshape(shape).astype(np.float32)
        # ... and what feeds the BN is scaled by gain per channel (conv1 for `_conv1`; conv2, its bias, the shortcut and
        # the projections for `_addition`; the dense layer for the position MLPs and `last_conv`)
        ea, eb = spec.emb_scopes(kind)
        q = (scope[:-len("_addition")] + "_conv2") if addition else scope
        # everything that is summed in front of this BN: the conv (and its bias), for the conditioned blocks the two
        # projections and the last layer of the two position MLPs, for `_addition` the `_transform` shortcut as well
        feeders = [q + "/w", q + "/b", q + ea + "/w", q + ea + "/b", q + eb + "/w", q + eb + "/b",
                   q + "_temb_dense3/w", q + "_femb_dense3/w"]
        if addition:
            feeders += [scope[:-len("_addition")] + "_transform/w", scope[:-len("_addition")] + "_transform/b"]
        if scope[-7:-1] == "_dense":                                          # doubled BN scopes of the position MLPs: S + S + "_denseN"
            feeders = [scope[(len(scope) - 7) // 2:] + "/w"]
        for f in feeders:
            if f in W:
                W[f] = (W[f].astype(np.float64) * gain.reshape((1,) * (W[f].ndim - 1) + (-1,))).astype(np.float32)
    return W


def tf_init(kind, s=51):
    W = {}
    for name, shape in spec.variable_shapes(kind).items():
        scope, leaf = name.rsplit("/", 1)
        r = _rng(s, name)
        if leaf == "w":
            if scope.endswith("_dense3") or scope.endswith("_emb") or scope == "last_dense":
                a = np.zeros(shape)
            else:
                a = r.normal(0.0, 0.01, size=shape)
                bad = np.abs(a) > 0.02                                        # truncated normal: redraw beyond 2 sigma
                while bad.any():
                    a[bad] = r.normal(0.0, 0.01, size=int(bad.sum()))
                    bad = np.abs(a) > 0.02
        elif leaf in ("b", "beta", "pop_mean"):
            a = np.zeros(shape)
        elif leaf in ("gamma", "pop_variance"):
            a = np.ones(shape)
        else:
            raise KeyError(name)
        W[name] = a.astype(np.float32)
    return W


LOUD_LOG2 = 5


def loud_scopes():
    """BatchNorm scope behind each of the 25 convs that write a stored tensor, in the library's numbering
    (NHANS_NUM_ACTIVATIONS), with the tensor's channel count."""
    out = []
    for i, g in enumerate(spec.tower_geometry() + spec.main_geometry()):
        p = ("embedding/" if i < 4 else "") + g["name"]
        out += [(p + "_conv1", g["cout"]), (p + "_addition", g["cout"])]
    return out + [("last_conv", 512)]


def loud_channel(j, C):
    """The loud channel of tensor j: the ends of the split layout's 32-channel hi / lo blocks, in turn."""
    return (0, 31, 32, C - 1)[j % 4]


def loud_readers(kind, j, W):
    """Weights that read tensor j, as (name, axis of the tensor's channel, its stride in that axis): conv2 of the block for a
    conv1 tensor; for a block output the next block's conv1 and `_transform`, for the tower's last the conditioning
    projections of every stack conv (the embedding is its mean), for the stack's last `last_conv`, then `last_dense` (NHWC
    flatten: row w * 512 + c).  The identity shortcut of the next block has no weight: blocks 1, 3, 5 and 7 of the stack."""
    blocks = ["embedding/" + g["name"] for g in spec.tower_geometry()] + [g["name"] for g in spec.main_geometry()]
    if j == 24:
        return [("last_dense/w", 0, 512)]
    p = blocks[j // 2]
    if j % 2 == 0:
        return [(p + "_conv2/w", 2, 1)]
    if j == 7:
        return [(k, 0, 1) for k in W if k.endswith("_emb/w") and not k.startswith("embedding/")]
    if j == 23:
        return [("last_conv/w", 2, 1)]
    q = blocks[j // 2 + 1]
    return [(q + "_conv1/w", 2, 1)] + ([(q + "_transform/w", 2, 1)] if q + "_transform/w" in W else [])


def one_channel_loud(kind, s=7, log2=LOUD_LOG2):
    """`synthetic7` with one output channel of every stored tensor 2^log2 times louder -- gamma and beta of the BatchNorm
    behind the conv times a power of two: exact in every format, and ReLU commutes with it --, channel loud_channel(j, C),
    and that input channel of every weight that reads the tensor (loud_readers) divided by the same power of two: every
    other figure of the network stays what it is in `synthetic7`, exactly, but for what an identity shortcut carries of a
    loud channel into the next block.  The maximum of each tensor then sits in a known channel
    (tests/test_calibration_checks_host.py asserts it in float64): a maximum kernel that skips part of a channel block
    cannot find it.  Not one of RECIPES: it exists for the calibration tests (tests/calibration_checks.py), the oracle
    comparison of tests/test_gpu_recipes.py has its weight sets."""
    W = dict(weights.synthetic_weights(kind, s))
    for j, (scope, C) in enumerate(loud_scopes()):
        c = loud_channel(j, C)
        for leaf in ("gamma", "beta"):
            a = W[scope + "/" + leaf].copy()
            assert a.reshape(-1).size == C, (scope, a.shape, C)
            a.reshape(-1)[c] *= np.float32(2.0 ** log2)
            W[scope + "/" + leaf] = a
        for name, axis, stride in loud_readers(kind, j, W):
            a = W[name].copy()
            assert a.shape[axis] == (C if stride == 1 else 26 * C) and stride in (1, C), (name, a.shape, C)
            idx = [slice(None)] * a.ndim
            idx[axis] = slice(c, None, stride) if stride > 1 else slice(c, c + 1)
            a[tuple(idx)] *= np.float32(2.0 ** -log2)
            W[name] = a
    return W


RECIPES = {
    "seed11": lambda kind: seed(kind, 11),
    "seed23": lambda kind: seed(kind, 23),
    "heavy": heavy,
    "trained_bn": trained_bn,
    "tf_init": tf_init,
}
