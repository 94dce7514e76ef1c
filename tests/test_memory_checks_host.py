"""tests/memory_checks.py on the CPU: the checker the device tests of tests/test_gpu_memory_contract.py rest on sees a
planted stray store, a planted hole and a read outside a range would change the input -- and only those."""
import numpy as np
import pytest

import memory_checks as MC

COUNTS = [5, 0, 1, 7]


def _written(kind, which, align, offsets, counts, value=1.5):
    g = MC.Guarded(kind, offsets[-1], align=align, which=which)
    for c, n in enumerate(counts):
        g.place(offsets[c], np.full(n, value + c))
    return g


@pytest.mark.parametrize("kind", sorted(MC.KINDS))
def test_layout_and_alignment(kind):
    la = MC.lanes(kind)
    assert MC.guard_elements(kind) * MC.itemsize(kind) == MC.GUARD * 4
    off = MC.ragged_offsets(list(range(la + 2)), kind)
    for c in range(la + 2):
        assert off[c] % la == c % la and off[c + 1] - off[c] >= c + 1          # every phase, room > count
    for align in range(la):
        g = MC.Guarded(kind, 11, align=align)
        assert g.ptr % 16 == align * MC.itemsize(kind)
        assert len(g.host_bits()) == 2 * MC.guard_elements(kind) + align + 11
        s = MC.Surrounded(kind, [np.ones(4)], [3], size=9, align=align)
        assert s.ptr % 16 == align * MC.itemsize(kind) and s.element_ptr(3) == s.ptr + 3 * MC.itemsize(kind)


@pytest.mark.parametrize("kind", sorted(MC.KINDS))
@pytest.mark.parametrize("align", [0, 1])
def test_checker_reports_planted_stores_and_holes(kind, align):
    off = MC.ragged_offsets(COUNTS, kind)
    mask = MC.prefix_mask(off, COUNTS)
    assert mask.sum() == sum(COUNTS) and not mask[off[0] + COUNTS[0]] and not mask[-1]
    untouched = MC.Guarded(kind, off[-1], align=align)
    f = MC.findings(untouched, mask, off)
    assert [x.what for x in f] == ["hole"] and f[0].count == sum(COUNTS) and f[0].first == 0 and f[0].clip == 0
    runs = [_written(kind, w, align, off, COUNTS) for w in (0, 1)]
    assert MC.findings(runs, mask, off) == [] and MC.findings(runs[0], mask, off) == []
    g = runs[0]
    plant = {"one word before the region": (g.front - 1, "guard_before", -1, None),
             "one word after the region": (g.front + g.size, "guard_after", 0, None),
             "the last guard word": (g.front + g.size + g.back - 1, "guard_after", g.back - 1, None),
             "the first guard word": (0, "guard_before", -g.front, None),
             "slack between clips 0 and 1": (g.front + off[0] + COUNTS[0], "slack", off[0] + COUNTS[0], 0),
             "slack of the empty clip": (g.front + off[1], "slack", off[1], 1),
             "the last slack element": (g.front + g.size - 1, "slack", g.size - 1, 3)}
    for name, (word, what, first, clip) in plant.items():
        hit = _written(kind, 0, align, off, COUNTS)
        hit.bits[word] = 0
        f = MC.findings([hit, runs[1]], mask, off)
        assert len(f) == 1 and f[0][:4] == (what, 1, first, clip), (name, f)
        assert "run 0" in f[0].text
    # distances are in 32-bit words, to the element's far end: two int16 next to the region share word 1, a double ends at 2
    hit = _written(kind, 0, align, off, COUNTS)
    hit.bits[g.front - 1] = 0
    hit.bits[g.front - 2] = 0
    assert "nearest %d words before" % (2 if kind == "f64" else 1) in MC.findings(hit, mask, off)[0].text
    # a hole at the last element of the last clip: that element holds each run's own sentinel
    last = off[3] + COUNTS[3] - 1
    holes = [_written(kind, w, align, off, COUNTS) for w in (0, 1)]
    for h in holes:
        h.bits[h.front + last] = h.sentinel
    f = MC.findings(holes, mask, off)
    assert len(f) == 1 and f[0][:4] == ("hole", 1, last, 3), f


def test_int16_output_equal_to_one_sentinel_is_no_hole():
    off = MC.ragged_offsets(COUNTS, "i16")
    mask = MC.prefix_mask(off, COUNTS)
    runs = [_written("i16", w, 3, off, COUNTS, value=MC.SENTINELS["i16"][0]) for w in (0, 1)]   # clip 0 "computes" 0x5AFE
    assert (runs[0].region()[:COUNTS[0]] == MC.SENTINELS["i16"][0]).all()
    alone = MC.findings(runs[0], mask, off)
    assert [x.what for x in alone] == ["hole"] and alone[0].count == COUNTS[0]        # one sentinel cannot tell
    assert MC.findings(runs, mask, off) == []                                       # two can
    assert MC.findings(runs[::-1], mask, off) == []


@pytest.mark.parametrize("kind,poison", [("f32", "nan"), ("f32", "big"), ("i16", "pcm")])
def test_input_variants_agree_inside_and_differ_outside(kind, poison):
    rng = np.random.default_rng(4)
    pieces = [rng.integers(-30000, 30000, n).astype(MC.KINDS[kind][0]) for n in (5, 0, 1, 7)]
    starts = [2, 9, 9, 13]
    for align in range(MC.lanes(kind)):
        a = MC.Surrounded(kind, pieces, starts, size=23, align=align, variant="A")
        b = MC.Surrounded(kind, pieces, starts, size=23, align=align, variant="B", poison=poison)
        wa, wb = a.host_bits(), b.host_bits()
        assert np.array_equal(a.inside, b.inside) and a.inside.sum() == 13
        assert np.array_equal(wa[a.inside], wb[a.inside])
        assert (wa[~a.inside] == 0).all() and (wa[~a.inside] != wb[~a.inside]).all()
        assert a.inside[a.front + 2] and not a.inside[a.front + 1] and not a.inside[a.front + 7] and not a.inside[a.front + 20]
        for p, s in zip(pieces, starts):
            assert MC.same_bits(b.region()[s:s + len(p)], p)
        out = b.region()[~b.inside[b.front:b.front + b.size]]
        if poison == "nan":
            assert np.isnan(out).all()
        elif poison == "big":
            assert (out == np.float32(1e30)).all()
        else:
            assert set(out.tolist()) == {32767, -32768} and (np.abs(np.diff(wb[:b.front].astype(np.int64))) == 65535).all()
