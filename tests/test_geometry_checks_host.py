"""The arithmetic of tests/geometry_checks.py, without a device: the committed table of batch geometries
(tests/golden/geometry_table.json) hits every reachable bucket of every launch kind of every arithmetic configuration,
the unreachable ones are listed with their reason, the 21-frame batch of tests/layer_checks.py hits what its docstring
says (and no more: the gap the table closes), and the comparison helper names the right tile, row and clip."""
import numpy as np
import pytest

import nhans_amd  # noqa: F401
from nhans_amd import hip, spec
import geometry_checks as G
import layer_checks as L
from test_row_classes_host import classes as lib_row_classes


@pytest.fixture(scope="module")
def table():
    return G.load_table()


@pytest.mark.parametrize("config", list(G.CONFIGS))
def test_table_hits_every_reachable_bucket(table, config):
    cfg = G.CONFIGS[config]
    uni, kinds = G.universe(cfg)
    reachable = {p for p, why in uni.items() if why is None}
    entries = table[config]["entries"]
    hit, rows = set(), []
    for i, e in enumerate(entries):
        assert set(e) == {"order", "fpc", "frame0", "nframes", "tensors", "name"}, e
        total = sum(G.POOL_FRAMES[c] for c in e["order"])
        assert 0 <= e["frame0"] and e["nframes"] >= 1 and e["frame0"] + e["nframes"] <= total, e
        assert max(n for _, n in G.tap_passes(e) + G.head_passes(e)) <= G.MAX_PASS, e
        assert all(8 <= t <= 24 for t in e["tensors"]), e
        h = G.entry_cover(cfg, e)
        new = (h & reachable) - hit
        rows.append("%3d  %4d frames in %3d clips  fpc %4d  tap [%3d, %3d)  tensors %-28s  +%3d pairs" % (
            i, total, len(e["order"]), e["fpc"], e["frame0"], e["frame0"] + e["nframes"], ",".join(map(str, e["tensors"])) or "-", len(new)))
        hit |= h
    by_bucket = {}
    for k, b in reachable:
        by_bucket.setdefault(b, [0, 0])[0] += 1
        by_bucket[b][1] += (k, b) in hit
    print("\n%s: %d launch kinds, %d reachable (kind, bucket) pairs, %d unreachable, %d entries" % (
        config, len(kinds), len(reachable), len(uni) - len(reachable), len(entries)))
    print("\n".join(rows))
    print("\n".join("  %-12s hit %3d of %3d" % (b, v[1], v[0]) for b, v in sorted(by_bucket.items())))
    missing = sorted(reachable - hit)
    assert not missing, "%d reachable pairs unhit, first: %s" % (len(missing), missing[:8])
    assert all(b in by_bucket for b in G.PASS_BUCKETS + G.CLIP_BUCKETS + ("r=0", "r<=2", "r>=tile-2", "M<tile", "grid<8"))
    # nothing is counted that the restatement does not know, and the unreachable pairs are the committed list, reasons included
    assert hit <= set(uni), sorted(hit - set(uni))[:8]
    assert not (hit - reachable), sorted(hit - reachable)[:8]
    want = sorted([k, b, why] for (k, b), why in uni.items() if why is not None)
    assert table[config]["unreachable"] == want
    assert all(why for _, _, why in want)


def test_every_mode_has_a_table(table):
    assert {c for _, _, c in G.MODES} == set(table) == set(G.CONFIGS)
    assert [m[1:] for m in G.MODES if m[2] in ("f16x3", "f32")] == [
        ("denoiser", "f16x3"), ("denoiser", "f32"), ("separator", "f16x3"), ("separator", "f32")]


def test_only_odd_residues_of_even_pixel_counts_and_grid_shapes_are_unreachable(table):
    """The size buckets that cannot be hit are those the issue's arithmetic predicts: a launch whose pixels per frame share a
    factor g with the tile reaches the multiples of g only; every other size bucket of every launch is reachable."""
    for config, cfg in G.CONFIGS.items():
        uni, kinds = G.universe(cfg)
        for (k, b), why in uni.items():
            l = kinds[k]
            if why is None or b not in G.SIZE_BUCKETS or b == "M<tile":
                continue
            g = int(np.gcd(l.px, l.tile))
            assert g > 1 and b != "r=0", (config, k, b, why)
            lo, hi = {"r<=2": (1, 2), "r>=tile-2": (l.tile - 2, l.tile - 1), "r~32": (30, 34), "r~64": (62, 66),
                      "r~tile/2": (l.tile // 2 - 2, l.tile // 2 + 2), "halo-1row": (1, l.wo)}.get(b, (0, -1))
            if b == "r~wave":
                assert all(v % g for m in G._wave_marks(l) for v in range(m - 2, m + 3)), (config, k, b)
            else:
                assert all(v % g for v in range(lo, hi + 1)), (config, k, b, g)


def test_row_classes_and_pixel_counts(lib_built):
    """The restated rule against the library's own (nhans_debug_row_classes), and the pixels per frame it gives."""
    lib = hip.load()
    for H, KH, s, pt in [(9, 3, 1, 1), (5, 3, 1, 1), (9, 3, 2, 1), (35, 4, 2, 1), (18, 3, 2, 0), (35, 4, 1, 1), (18, 4, 1, 1)]:
        n, cl = lib_row_classes(lib, H, KH, s, pt)
        assert G.row_classes(H, KH, s, pt) == cl, (H, KH, s, pt)
    px = sorted({g["hout"] * g["wout"] for g in spec.activation_geometry()[8:24]}, reverse=True)
    assert px == [7035, 1818, 459, 130]
    by_conv = {}
    for l in G.stack_launches(G.CONFIGS["f16x3"], 1, 1):
        by_conv.setdefault(l.conv, []).append(l.px)
    assert by_conv["resblock3_2_conv1"] == [51, 357, 51] and by_conv["resblock3_1_conv2"] == [51, 357, 51]
    assert by_conv["resblock4_2_conv2"] == [26, 78, 26] and by_conv["resblock4_1_conv1"] == [26, 78, 26]
    assert by_conv["resblock3_1_conv1"] == [459] and by_conv["resblock2_1_conv1"] == [1818]       # row_split 1: do not pay
    two = {}
    for l in G.stack_launches(G.CONFIGS["f16x3"], 1, 2):
        two.setdefault(l.conv, []).append(l.px)
    assert two["resblock2_1_conv1"] == [101, 1616, 101] and two["resblock3_1_conv1"] == [408, 51]
    # the f32 path and the variants below 2 are never split
    for config in ("f32", "f16x3 conv_variant=0", "f16x3 conv_variant=1"):
        assert all(not l.cls for l in G.stack_launches(G.CONFIGS[config], 3, 2)), config


def test_the_layer_batch_hits_what_its_docstring_says():
    """tests/layer_checks.py: 21 frames, one launch and passes of 8 -- the residues its comment lists, every last tile
    ragged; and what that leaves out: no full last tile, none of one or two rows, none two short of full."""
    L.check_batch_geometry()
    want = {7035: (23, 23, 279), 1818: (34, 34, 290), 459: (39, 167, 423), 130: (42, 170, 170)}
    for px, res in want.items():
        assert tuple((L.TOTAL * px) % t for t in L.TILES) == res
    seen = set()
    for config in ("f32", "f16x3 winograd=0"):
        for rs in G.row_splits(G.CONFIGS[config]):
            for n in (21, 8, 5):
                for l in G.stack_launches(G.CONFIGS[config], n, rs):
                    if l.per_frame or l.tensor == G.HEADS_TENSOR:
                        continue
                    if n == 21 and not l.cls and l.px in want:
                        assert l.M % l.tile == want[l.px][L.TILES.index(l.tile)], l
                    if not l.cls:
                        assert l.M % l.tile, l                      # "the last tile of every launch is ragged"
                        if n == 21:
                            seen |= G.size_buckets(l)
    # the launch of all 21 frames: no full last tile, none of one or two rows, none two short, none below a tile (its
    # passes of 8 and 5 frames add what 5 x 1,818 = 2 mod 128 and 5 x 26 = 130 < 256 happen to give, on three layers)
    assert not seen & {"r=0", "r<=2", "r>=tile-2", "M<tile"}, seen
    # the clip edges it does have: a one-frame clip between two others, a pass boundary inside a clip
    e = dict(order=[0, 1, 2], fpc=L.CHUNK, frame0=0, nframes=L.TOTAL, tensors=list(range(8, 25)), name="")
    hit = G.entry_cover(G.CONFIGS["f16x3"], e)
    assert {b for _, b in hit} & set(G.PASS_BUCKETS) == {"pass starts in a clip", "pass ends in a clip"}
    assert not any(b == "4clips" for _, b in hit)


def test_difference_is_located_in_the_last_partial_tile():
    """A 9-frame clip and a one-frame clip after it: the top row class of resblock4_2's conv2 is M = 10 x 26 = 260 pixels,
    one full 256-pixel tile and a last tile of 4 rows that belong to the one-frame clip."""
    cfg = G.CONFIGS["f16x3"]
    e = dict(order=[2, 1], fpc=3776, frame0=0, nframes=10, tensors=[23], name="")
    g = spec.activation_geometry()[23]
    rng = np.random.default_rng(1)
    want = rng.standard_normal((10, g["hout"], g["wout"], g["cout"])).astype(np.float32)
    assert G.describe_difference(cfg, e, 1, 23, want.copy(), want, np.arange(10)) is None
    got = want.copy()
    got[9, 0, 23, 5] += 1.0
    (l, tile, row, g0), = G.locate(cfg, e, 1, 23, 9, 0, 23)
    assert (l.conv, l.kernel, l.cls, l.M, l.tile, tile, row, g0) == ("resblock4_2_conv2", "conv_igemm_halo<128>", "rows 0..0", 260, 256, 1, 1, 0)
    msg = G.describe_difference(cfg, e, 1, 23, got, want, np.arange(10))
    for part in ("tensor 23 (stack resblock4_2 output)", "1 of %d elements" % want.size, "first at frame 9 (frame 0 of clip instance 1 = pool clip 1, 1 frames)",
                 "pixel (h 0, w 23), channel 5", "resblock4_2_conv2 conv_igemm_halo<128> rows 0..0 M 260 tile 256: tile 1 of 2 (the partial last tile, 4 rows), row 1 of it"):
        assert part in msg, (part, msg)
    # the same element without the row classes: one launch of M = 1300, tile 5 of 6, row 1234 - 1280 + ... = 9 * 130 + 23 - 5 * 256
    (l, tile, row, g0), = G.locate(cfg, e, 0, 23, 9, 0, 23)
    assert (l.cls, l.M, tile, row) == ("", 1300, 4, 9 * 130 + 23 - 4 * 256)
    # interior row of the image, second pass of a chunked fetch, and the head rows
    e2 = dict(order=[2, 1], fpc=4, frame0=1, nframes=9, tensors=[23], name="")
    (l, tile, row, g0), = G.locate(cfg, e2, 1, 23, 6, 2, 3)
    assert (l.cls, l.M, g0, tile, row) == ("rows 1..3", 4 * 78, 5, 0, 78 + 26 + 3)
    rows = rng.standard_normal((10, 201)).astype(np.float32)
    bad = rows.copy()
    bad[7, 100] = 0.0
    bad[8, 3] = 0.0
    msg = G.describe_difference(cfg, e, 1, G.HEADS_TENSOR, bad, rows, np.arange(10), heads=True)
    assert "2 of 2010 elements" in msg and "first at frame 7" in msg and "channel 100" in msg and "last_dense conv_igemm_dma<128,grouped> M 10 tile 256: tile 0 of 1" in msg, msg


def test_tower_cases_cover_what_nine_images_can_reach():
    for config in ("f16x3", "f32"):
        cases, total = G.tower_cases(G.CONFIGS[config])
        assert cases and all(1 <= cpc <= n <= G.TOWER_MAX for n, cpc in cases)
        buckets = {b for _, b in total}
        # passes of one to nine images of 6,767 / 1,173 / 598 pixels reach few residues: a last tile of two rows (3 x 598 =
        # 2 mod 128 and 256), one two short of full, one at a wave boundary, and every shape of grid the XCD remap splits
        assert {"r<=2", "r>=tile-2", "r~wave", "grid%8=0", "grid%8=1", "grid%8=7"} <= buckets, (config, buckets)
        sizes = {min(cpc, n - g0) for n, cpc in cases for g0 in range(0, n, cpc)}
        assert any(cpc < n for n, cpc in cases) and len(sizes) >= 5, cases
        print(config, cases, len(total))
