"""Option row_split (host_net.hip: run_conv_row_classes): the 3x3 convs of resblock3 / resblock4 as one launch per class of
output rows, each with only the filter rows that touch the image.  The filter rows left out multiplied SAME padding --
exact zeros into the same f32 accumulator in the same order -- so row_split = 1 must give the bits of row_split = 0 (the
single launch) in every stored tensor from resblock3_1 on (16 .. 24), in the logits and in the denoised rows."""
import numpy as np
import pytest
import torch

import nhans_amd  # noqa: F401
from nhans_amd import engine

pytestmark = pytest.mark.gpu

TENSORS = range(16, 25)         # conv1 / block outputs of resblock3_1 .. resblock4_2, last_conv


@pytest.fixture(scope="module")
def _eng_d(lib_built, weights_denoiser):
    e = engine.Engine("denoiser", weights_denoiser)
    yield e
    e.close()


@pytest.fixture(scope="module")
def _eng_s(lib_built, weights_separator):
    e = engine.Engine("separator", weights_separator)
    yield e
    e.close()


def batch(nfr, seed):
    g = torch.Generator().manual_seed(seed)
    lm = (torch.randn(sum(nfr), 201, generator=g) * 2.0 - 4.0).cuda()
    ea = (torch.randn(len(nfr), 512, generator=g) * 0.1).cuda()
    eb = (torch.randn(len(nfr), 512, generator=g) * 0.1).cuda()
    return lm, [int(v) for v in np.concatenate([[0], np.cumsum(nfr)])], ea, eb


def run(eng, value, lm, foff, ea, eb, tensors=TENSORS):
    eng.set_option("row_split", value)
    out = {i: eng.activation(i, lm, foff, ea, eb, 0, foff[-1]).cpu().numpy() for i in tensors}
    lg, den = eng.mask_net(lm, foff, ea, eb)
    out["logits"], out["denoised"] = lg.cpu().numpy(), den.cpu().numpy()
    assert eng.take_status() == 0
    return out


def assert_same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].shape == b[k].shape and np.isfinite(a[k]).all(), k
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


def compare(eng, nfr, seed, prec="f16x3", wino=1, chunk=3776, values=(1,), tensors=TENSORS):
    eng.set_precision(prec)
    lm, foff, ea, eb = batch(nfr, seed)
    try:
        eng.set_option("winograd", wino)
        eng.set_option("frames_per_chunk", chunk)
        ref = run(eng, 0, lm, foff, ea, eb, tensors)
        for v in values:
            assert_same_bits(ref, run(eng, v, lm, foff, ea, eb, tensors))
    finally:
        eng.set_option("row_split", 1)
        eng.set_option("winograd", 1)
        eng.set_option("frames_per_chunk", 3776)
        eng.set_precision("f16x3")
    return ref


def test_one_frame_every_class_smaller_than_a_tile(_eng_d):
    """One clip of one frame: the one-row classes are 26 and 51 pixels, the interior ones 78 and 357."""
    compare(_eng_d, [1], 3)


@pytest.mark.parametrize("chunk", [8, 3776])
@pytest.mark.parametrize("wino", [1, 0])
@pytest.mark.parametrize("kind", ["denoiser", "separator"])
def test_three_clips_in_one_call(_eng_d, _eng_s, kind, wino, chunk):
    """Clips of 11 + 1 + 9 frames: a one-row class tile of 256 pixels spans about 10 frames (5 at 51 columns) and crosses
    both clip boundaries, so its bias rows are per pixel, not hoisted; at 8 frame windows per pass a chunk boundary lies
    inside the first and the last clip."""
    compare(_eng_d if kind == "denoiser" else _eng_s, [11, 1, 9], 5, wino=wino, chunk=chunk)


def test_partial_last_tile_in_the_one_row_classes(_eng_d):
    """257 frames: 257 x 26 and 257 x 51 pixels per one-row class, neither a multiple of the 256-pixel tile."""
    compare(_eng_d, [257], 7)


def test_every_conv_that_can_be_split(_eng_d):
    """row_split = 2, the measurement value: the strided convs of resblock2_1 / resblock3_1 (pointwise mode; two classes for
    the 18 -> 9 one) are split as well -- tensors from resblock2_1's conv1 on."""
    compare(_eng_d, [11, 1, 9], 9, values=(2,), tensors=range(12, 25))
    compare(_eng_d, [3], 9, wino=0, values=(2,), tensors=range(12, 25))


def test_f32_precision_is_not_split(_eng_d):
    """The f32 path is never split: the option changes no bit and no launch."""
    compare(_eng_d, [11, 1, 9], 11, prec="f32", values=(1, 2))
    _eng_d.set_precision("f32")
    lm, foff, ea, eb = batch([4], 11)
    calls = {}
    try:
        _eng_d.set_option("profile", 1)
        for v in (0, 1):
            _eng_d.set_option("row_split", v)
            _eng_d.profile_reset()
            _eng_d.mask_net(lm, foff, ea, eb)
            calls[v] = {k: e["calls"] for k, e in _eng_d.profile().items()}
    finally:
        _eng_d.set_option("profile", 0)
        _eng_d.set_option("row_split", 1)
        _eng_d.set_precision("f16x3")
    assert calls[0] == calls[1]


def test_profile_shows_three_launches_per_split_conv_on_the_same_flops(_eng_d):
    """One call: the six stride-1 3x3 convs of resblock3 / resblock4 (conv_igemm_halo<128>) and resblock4_1's strided conv1
    (pointwise mode) run as three launches each under their kernel's unchanged name.  `flops` stands for the direct
    convolutions the launches compute and sums to the single launches' figure exactly; `mfma_flops` is what ran: 25 / 27
    and 13 / 15 of the filter rows."""
    _eng_d.set_precision("f16x3")
    lm, foff, ea, eb = batch([11, 1, 9], 13)
    prof = {}
    try:
        _eng_d.set_option("profile", 1)
        for v in (0, 1):
            _eng_d.set_option("row_split", v)
            _eng_d.profile_reset()
            _eng_d.mask_net(lm, foff, ea, eb)
            prof[v] = _eng_d.profile()
    finally:
        _eng_d.set_option("profile", 0)
        _eng_d.set_option("row_split", 1)
    assert prof[0].keys() == prof[1].keys()
    split = {"conv_igemm_halo<128>": 6, "conv_igemm_halo_pw<128>": 1}
    for k in prof[0]:
        a, b = prof[0][k], prof[1][k]
        assert b["calls"] == a["calls"] + 2 * split.get(k, 0), (k, a, b)
        assert b["flops"] == a["flops"], (k, a, b)
        if k in split:
            assert b["mfma_flops"] < a["mfma_flops"], (k, a, b)
        else:
            assert b["mfma_flops"] == a["mfma_flops"], (k, a, b)
    # conv_igemm_halo<128> is exactly those six convs: per frame window 3 x 270.7 + 3 x 306.7 MMAC, of which 60.2 + 122.7 go
    a, b = prof[0]["conv_igemm_halo<128>"], prof[1]["conv_igemm_halo<128>"]
    full = 3 * 9 * 51 * 9 * 256 * 256 + 9 * 51 * 128 * 256 + 3 * 5 * 26 * 9 * 512 * 512 + 5 * 26 * 256 * 512
    gone = 3 * 2 * 51 * 3 * 256 * 256 + 3 * 2 * 26 * 3 * 512 * 512
    assert a["flops"] == pytest.approx(2.0 * 21 * full, rel=2e-6)
    assert a["mfma_flops"] - b["mfma_flops"] == pytest.approx(3 * 2.0 * 21 * gone, rel=1e-4)
