"""Batch geometries at every conv tile edge (tests/test_gpu_geometry.py on the device, tests/test_geometry_checks_host.py
for the arithmetic of this file): a pool of clips with float64 / float32 CPU references, a restatement of the conv
launches one pass of the stack or the tower makes, the buckets a launch falls into, the committed table of geometries
that hits every bucket (tests/golden/geometry_table.json, built by tools/geometry_cover.py) and the comparison that says
WHERE two fetches of one tensor differ.  Nothing here touches the device.

The contract under test: the bits of a frame do not depend on where the frame sits in a batch or a pass.  So a clip run
alone -- held to float64 at layer_checks.BAR -- is the reference for the same clip anywhere, bit for bit.

Where the restatement was read:
  which kernel runs a conv      conv_igemm.hip launch_conv_igemm() (the order of its tests), conv_igemm_halo.hip
                                conv_igemm_halo_eligible() / conv_igemm_halo_pw_eligible(), conv_wino.hip
                                conv_wino_eligible(), net_weights.h (which convs have a Winograd pack), host_net.hip
                                run_stack_chunk() / embed_impl() / stack_and_head() (kgroup = -1, the stand-alone transform)
  tile and grid of a kernel     the launchers: conv_igemm.hip launch_t (BM 128), conv_igemm_dma.hip launch_dma_t (DBM 256),
                                conv_igemm_halo.hip launch_halo_t (HaloShape::HBM 256 / 512), conv_wino.hip launch_wino_t +
                                wino_block (per frame), conv_1x1_stream.hip (4 waves x 32 pixels, grid capped at 512),
                                aux_kernels.hip launch_direct_conv64 (the 4x4 kernel: 13 strips per frame, grid capped at
                                2,048; the generic one: 16 pixels per workgroup, capped at 4,096)
  row classes                   host_net.hip row_classes(), row_split_pays(), run_conv_row_classes(), halo_family()

Granularities of the guard code besides the buckets the tile size gives (r = M mod tile):
  * every kernel tests `m < a.M` per pixel row; conv_igemm stages rows (tid >> 3) + 32 i and its waves own 64 (BN 128) or 32
    (BN 64) rows: the multiples of 32 up to the tile.  The halo / DMA kernels' consumer waves own 64 rows each (4 or 8
    along the pixels): the multiples of 64 up to the tile.  32, 64 and tile / 2 are buckets of their own; the other
    multiples are the bucket `r~wave`.  conv_1x1_stream: a wave's group is 32 pixels, a store instruction two.
  * conv_epilogue.h sweeps a tile in passes of NTHREADS / (BN / 4) or, split-f16 with epilogue_wide, NTHREADS / (BN / 8)
    pixels -- 8, 16, 32 or 64 --, and fills the slots past the end with the LAST valid pixel.  Every pass boundary is a
    multiple of 8; the +-2 windows at 32, 64, tile / 2 and the wave multiples straddle one, 1 <= r <= 2 leaves all
    passes but the first empty, r >= tile - 2 leaves the last pass two pixels short.
  * the halo kernel (not its pointwise mode) stages image rows: its last tile holds r / Wo of them.  `halo-1row`: the last
    tile lies within one image row (r <= Wo).
  * a kernel whose grid is capped walks more than one tile per workgroup beyond the cap: `capped`.
  * conv_wino and the stack's direct_conv64 tile every frame alone: only their grid depends on the pass.
"""
import json
import os
from collections import namedtuple

import numpy as np

import nhans_amd  # noqa: F401
from nhans_amd import spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE_PATH = os.path.join(ROOT, "tests", "golden", "geometry_table.json")
MAX_PASS = 512                      # frame windows per pass the table may ask for

# ---- the arithmetic configurations (geometry does not depend on the model kind) ----------------------------------------
# variant: ConvArgs::variant as host_net.hip fill_epilogue_defaults() resolves option conv_variant (-1: 2 in f16x3, 0 in f32)
Config = namedtuple("Config", "prec variant wino options")
CONFIGS = {
    "f16x3": Config("f16x3", 2, True, {}),
    "f16x3 winograd=0": Config("f16x3", 2, False, {"winograd": 0}),
    "f16x3 conv_variant=0": Config("f16x3", 0, False, {"conv_variant": 0}),
    "f16x3 conv_variant=1": Config("f16x3", 1, False, {"conv_variant": 1}),
    "f32": Config("f32", 0, False, {}),
}
# (test id, model kind, configuration)
MODES = [("denoiser f16x3", "denoiser", "f16x3"), ("denoiser f16x3 winograd=0", "denoiser", "f16x3 winograd=0"),
         ("denoiser f16x3 conv_variant=0", "denoiser", "f16x3 conv_variant=0"),
         ("denoiser f16x3 conv_variant=1", "denoiser", "f16x3 conv_variant=1"), ("denoiser f32", "denoiser", "f32"),
         ("separator f16x3", "separator", "f16x3"), ("separator f32", "separator", "f32")]


def row_splits(cfg):
    """The values of option row_split whose launches differ in this configuration (f32 is never split; below variant 2
    nothing is in the halo family)."""
    return (1, 0, 2) if cfg.prec == "f16x3" and cfg.variant >= 2 else (1,)


# ---- the kernels: pixels per workgroup tile, output channels per workgroup --------------------------------------------
# tile 0: the kernel tiles each frame on its own
KERNEL_TILE = {
    "conv_igemm<64>": (128, 64), "conv_igemm<128>": (128, 128),
    "conv_igemm_dma<64>": (256, 64), "conv_igemm_dma<128>": (256, 128),
    "conv_igemm_dma<64,grouped>": (256, 64), "conv_igemm_dma<128,grouped>": (256, 128),
    "conv_igemm_halo<64,512>": (512, 64), "conv_igemm_halo<64>": (256, 64), "conv_igemm_halo<128>": (256, 128),
    "conv_igemm_halo_pw<128>": (256, 128),
    "conv_wino<128>": (0, 64),
    "conv_1x1_stream": (128, 128),
    "direct_conv64": (16, 64),          # the generic kernel (tower); the stack's 4x4 kernel tiles per frame (tile 0)
}
GRID_CAP = {"conv_1x1_stream": 512, "direct_conv64": 4096, "direct_conv64 4x4": 2048}
HALO_ROWS = {256: 320, 512: 544}        # HaloShape::HR

# tensor: index of the stored tensor the launch writes (25: logits / denoised rows); conv: the layer; kernel: the name
# the profile shows; cls: "" or the output rows of a row-class launch; px: pixels per frame in THIS launch; wo: image
# width; oh0 / rows: the output rows it covers; M, tile, grid; per_frame: tiles never cross frames
Launch = namedtuple("Launch", "tensor conv kernel cls px wo oh0 rows M tile grid per_frame capped")
HEADS_TENSOR = 25


def row_classes(H, KH, s, pt):
    """host_net.hip row_classes(): [(oh0, rows, kh0, kh)], [] if some output row reads padding only."""
    out = []
    for ho in range(-(-H // s)):
        hi0 = ho * s - pt
        lo, hi = max(0, -hi0), min(KH, H - hi0)
        if hi <= lo:
            return []
        if out and out[-1][2] == lo and out[-1][3] == hi - lo:
            out[-1][1] += 1
            continue
        out.append([ho, 1, lo, hi - lo])
    return [tuple(c) for c in out]


def row_split_pays(KH, classes):
    applied = sum(r * k for _, r, _, k in classes)
    rows = sum(r for _, r, _, _ in classes)
    return 100 * (rows * KH - applied) >= 7 * rows * KH


def wino_block(Ho, ntile, KH=4, m=5):
    """conv_wino.hip wino_block(): (rows, tiles) of a workgroup's block of tile-pixels."""
    best, tr, tj = -1.0, 0, 0
    for r in range(1, 129):
        t = 1
        while r * t <= 128:
            ok = not (r + KH - 1 > 21 or t * m + KH - 1 > 38 or 128 + (KH - 1) * t > 152 or (r + KH - 1) * t * 2 > 512)
            if ok:
                nrb, ncb = -(-Ho // r), -(-ntile // t)
                u = float(Ho) * ntile / (float(nrb) * ncb * 128) - 0.02 * float(r + KH - 1) / r
                if u > best:
                    best, tr, tj = u, r, t
            t += 1
    return tr, tj


_wino_wgs = {}


def wino_workgroups_per_frame(Ho, Wo, N):
    if (Ho, Wo, N) not in _wino_wgs:
        ntile = -(-Wo // 5)
        tr, tj = wino_block(Ho, ntile)
        _wino_wgs[(Ho, Wo, N)] = -(-Ho // tr) * -(-ntile // tj) * (N // 64)
    return _wino_wgs[(Ho, Wo, N)]


def _halo_fits(tile, Wo, KW):
    nrows = (Wo - 1 + tile - 1) // Wo + 1
    return tile + (KW - 1) * nrows <= HALO_ROWS[tile]


def choose_kernel(cfg, KH, KW, sw, C, N, nseg, kgroup, wino_pack, Wo, same=True):
    """launch_conv_igemm()'s choice for one conv.  same: SAME padding (with sw == 1 then Wo == W)."""
    wide = N % 128 == 0
    if cfg.variant == 0:
        return "conv_igemm<128>" if wide else "conv_igemm<64>"
    halo_ok = cfg.variant >= 2 and kgroup == 0
    if halo_ok and cfg.wino and cfg.prec == "f16x3" and wino_pack and nseg == 1:
        return "conv_wino<128>"
    halo = halo_ok and same and KW >= 3 and sw == 1
    if halo and not wide and _halo_fits(512, Wo, KW):
        return "conv_igemm_halo<64,512>"
    if halo and _halo_fits(256, Wo, KW):
        return "conv_igemm_halo<128>" if wide else "conv_igemm_halo<64>"
    if halo_ok and wide and nseg == 1 and C % 32 == 0 and KH * KW * (C // 32) >= 4:
        return "conv_igemm_halo_pw<128>"
    g = ",grouped" if kgroup < 0 else ""
    return "conv_igemm_dma<128%s>" % g if wide else "conv_igemm_dma<64%s>" % g


def _launch(tensor, conv, kernel, n, px, wo, oh0=0, rows=0, cls="", N=64):
    tile, bn = KERNEL_TILE[kernel]
    M = n * px
    cap = GRID_CAP.get(kernel)
    if tile == 0:
        grid = n * wino_workgroups_per_frame(rows, wo, N)
        return Launch(tensor, conv, kernel, cls, px, wo, oh0, rows, M, 0, grid, True, False)
    if kernel == "conv_1x1_stream":
        groups = -(-M // 32)
        full = -(-groups // 4)
        return Launch(tensor, conv, kernel, cls, px, wo, oh0, rows, M, tile, min(cap, full), False, full > cap)
    full = -(-M // tile) * (1 if kernel == "direct_conv64" else N // bn)
    grid = min(cap, full) if cap else full
    return Launch(tensor, conv, kernel, cls, px, wo, oh0, rows, M, tile, grid, False, bool(cap) and full > cap)


def _conv_launches(cfg, row_split, tensor, conv, n, H, Ho, Wo, KH, KW, sh, sw, C, N, nseg, wino_pack):
    """One conv of the stack as run_stack_chunk()'s conv() makes it: the single launch, or one per row class."""
    kernel = choose_kernel(cfg, KH, KW, sw, C, N, nseg, 0, wino_pack, Wo)
    if (row_split and cfg.prec == "f16x3" and cfg.variant >= 2 and N % 128 == 0
            and kernel in ("conv_igemm_halo<128>", "conv_igemm_halo_pw<128>")):
        pt = max((Ho - 1) * sh + KH - H, 0) // 2
        rc = row_classes(H, KH, sh, pt)
        if len(rc) >= 2 and (row_split == 2 or row_split_pays(KH, rc)):
            return [_launch(tensor, conv, kernel, n, r * Wo, Wo, oh0, r, "rows %d..%d" % (oh0, oh0 + r - 1), N)
                    for oh0, r, _, _ in rc]
    return [_launch(tensor, conv, kernel, n, Ho * Wo, Wo, 0, Ho, "", N)]


def stack_launches(cfg, n, row_split=1):
    """Every conv launch of one pass of n frame windows through the stack and head, in launch order."""
    out = []
    for b, g in enumerate(spec.main_geometry()):
        t1, t2 = 8 + 2 * b, 9 + 2 * b
        name, k, Ho, Wo, co, ci = g["name"], g["kh"], g["hout"], g["wout"], g["cout"], g["cin"]
        if b == 0:
            # the 4x4 stride-1 kernel: strips of 35 rows x 16 pixels, 13 per frame
            strips = n * -(-Wo // 16)
            cap = GRID_CAP["direct_conv64 4x4"]
            out.append(Launch(t1, name + "_conv1", "direct_conv64", "", Ho * Wo, Wo, 0, Ho, n * Ho * Wo, 0, min(strips, cap),
                              True, strips > cap))
        else:
            pack = k == 4 and g["sh"] == 1 and ci == co
            out += _conv_launches(cfg, row_split, t1, name + "_conv1", n, g["hin"], Ho, Wo, k, k, g["sh"], g["sw"], ci, co, 1, pack)
        changing = ci != co and ci > 1
        wino2 = cfg.variant >= 2 and cfg.wino and cfg.prec == "f16x3" and k == 4
        if changing and wino2:
            # the 1x1 strided `_transform` conv on its own, then conv2 in its Winograd form
            out.append(_launch(t2, name + "_transform", "conv_1x1_stream", n, Ho * Wo, Wo, 0, Ho, "", co))
        nseg = 2 if changing and not wino2 else 1
        out += _conv_launches(cfg, row_split, t2, name + "_conv2", n, Ho, Ho, Wo, k, k, 1, 1, co, co, nseg, k == 4)
    g = spec.main_geometry()[-1]
    kern = choose_kernel(cfg, g["hout"], 1, 1, 512, 512, 1, 0, False, g["wout"], same=False)
    out.append(_launch(24, "last_conv", kern, n, g["wout"], g["wout"], 0, 1, "", 512))
    kern = choose_kernel(cfg, 1, 1, 1, g["wout"] * 512, 256, 1, -1, False, 1, same=False)
    out.append(_launch(HEADS_TENSOR, "last_dense", kern, n, 1, 1, 0, 1, "", 256))
    return out


def tower_launches(cfg, n):
    """Every conv launch of one pass of n context images through the embedding tower (embed_impl())."""
    out = []
    for b, g in enumerate(spec.tower_geometry()):
        name, Ho, Wo, co = g["name"], g["hout"], g["wout"], g["cout"]
        if b == 0:
            out.append(_launch(0, name + "_conv1", "direct_conv64", n, Ho * Wo, Wo, 0, Ho, "", co))
        else:
            kern = choose_kernel(cfg, g["kh"], g["kw"], g["sw"], g["cin"], co, 1, -1, False, Wo)
            out.append(_launch(2 * b, name + "_conv1", kern, n, Ho * Wo, Wo, 0, Ho, "", co))
        kern = choose_kernel(cfg, g["kh"], g["kw"], 1, co, co, 2 if g["cin"] > 1 else 1, 0, False, Wo)
        out.append(_launch(2 * b + 1, name + "_conv2", kern, n, Ho * Wo, Wo, 0, Ho, "", co))
    return out


def kind_of(l):
    """What the cover counts: one layer's launch on one kernel (and one row class)."""
    return "%s %s%s" % (l.conv, l.kernel, " " + l.cls if l.cls else "")


def profile_calls(cfg, passes, row_split=1):
    """{profile name: calls} of one nhans_mask_net call whose passes have the given sizes: every conv launch of the stack and
    head, and the conditioning projection once."""
    calls = {"cond_proj": 1}
    for n in passes:
        for l in stack_launches(cfg, n, row_split):
            calls[l.kernel] = calls.get(l.kernel, 0) + 1
    return calls


# ---- buckets -----------------------------------------------------------------------------------------------------
SIZE_BUCKETS = ("M<tile", "r=0", "r<=2", "r~32", "r~64", "r~tile/2", "r>=tile-2", "r~wave", "halo-1row")
GRID_BUCKETS = ("grid<8", "grid%8=0", "grid%8=1", "grid%8=7", "capped")
CLIP_BUCKETS = ("4clips", "end+1f")
# of every launch of a pass (the per-frame kernels too: the clip map and the window rows of a pass that cuts a clip)
PASS_BUCKETS = ("pass starts in a clip", "pass ends in a clip", "frame0>0")


def _wave_marks(l):
    step = 32 if l.tile == 128 else 64
    return [v for v in range(step, l.tile, step) if v not in (32, 64, l.tile // 2)]


def applicable(l):
    """The buckets that mean something for this launch kind."""
    out = ["grid<8", "grid%8=0", "grid%8=1", "grid%8=7"]
    if l.kernel in GRID_CAP or (l.kernel == "direct_conv64" and l.per_frame):
        out.append("capped")
    if l.per_frame:
        return out
    out += ["M<tile", "r=0", "r<=2", "r>=tile-2"]
    if l.tile > 34:
        out.append("r~32")
    if l.tile > 66:
        out.append("r~64")
    if l.tile // 2 not in (32, 64) and l.tile >= 8:
        out.append("r~tile/2")
    if _wave_marks(l):
        out.append("r~wave")
    if l.kernel.startswith("conv_igemm_halo<"):
        out.append("halo-1row")
    return out + list(CLIP_BUCKETS)


def size_buckets(l):
    """The size and grid buckets launch l is in."""
    hit = set()
    if l.grid < 8: hit.add("grid<8")
    if l.grid % 8 in (0, 1, 7): hit.add("grid%%8=%d" % (l.grid % 8))
    if l.capped: hit.add("capped")
    if l.per_frame:
        return hit
    r = l.M % l.tile
    if l.M < l.tile: hit.add("M<tile")
    if r == 0: hit.add("r=0")
    if 1 <= r <= 2: hit.add("r<=2")
    if r and r >= l.tile - 2: hit.add("r>=tile-2")
    near = lambda v: r and abs(r - v) <= 2
    if l.tile > 34 and near(32): hit.add("r~32")
    if l.tile > 66 and near(64): hit.add("r~64")
    if l.tile // 2 not in (32, 64) and near(l.tile // 2): hit.add("r~tile/2")
    if any(near(v) for v in _wave_marks(l)): hit.add("r~wave")
    if l.kernel.startswith("conv_igemm_halo<") and 1 <= r <= l.wo: hit.add("halo-1row")
    return hit & set(applicable(l))


def clip_buckets(l, cid, clen):
    """The clip-edge buckets of launch l over a pass whose frame i belongs to clip instance cid[i] (ascending) of clen[i]
    frames: a tile with rows of four or more clips; a partial last tile with the end of one clip and a one-frame clip
    after it."""
    hit = set()
    if l.per_frame:
        return hit
    n = len(cid)
    starts = np.arange(0, l.M, l.tile, dtype=np.int64)
    f0 = starts // l.px
    f1 = (np.minimum(starts + l.tile, l.M) - 1) // l.px
    if int((cid[f1] - cid[f0]).max()) >= 3:
        hit.add("4clips")
    if l.M % l.tile and n >= 2 and clen[n - 1] == 1 and cid[n - 1] != cid[n - 2] and cid[f0[-1]] != cid[n - 1]:
        hit.add("end+1f")
    return hit


def max_frames_in_tile(l):
    return (l.tile - 2) // l.px + 2 if l.tile >= 2 else 1


def clip_reachable(l, bucket):
    """4clips: a tile can touch four frames.  end+1f: the partial last tile can reach back past the last frame."""
    if l.per_frame:
        return False
    return max_frames_in_tile(l) >= 4 if bucket == "4clips" else l.px < l.tile - 1


# ---- the pool of clips -------------------------------------------------------------------------------------------
# clips 0 .. 2 are layer_checks' (11, 1 and 9 frames, conditioning pairs (0,1), (1,2), (2,0) of its three contexts); two more
# one-frame clips and a two-frame clip take the other three ordered pairs: no two pool clips share a pair
POOL_FRAMES = (11, 1, 9, 1, 1, 2)
POOL_PAIRS = ((0, 1), (1, 2), (2, 0), (1, 0), (2, 1), (0, 2))
POOL_SEEDS = (61, 62, 63, 71, 72, 73)
ONE_FRAME = tuple(i for i, f in enumerate(POOL_FRAMES) if f == 1)


class ClipRef:
    """acts {8..24: tensor [frames,H,W,C]}, logits, denoised [frames,201] of one pool clip in one dtype."""


def pool_features():
    """([201-bin log-magnitude rows of each pool clip], contexts [3,200,201]) as float32; clips 0..2 are layer_checks'."""
    import layer_checks as L
    from nhans_amd import apply, synth
    import oracle.nhans_oracle as O
    lms, ctx = L.features()
    for seed, nfr in list(zip(POOL_SEEDS, POOL_FRAMES))[3:]:
        mix = apply.trim_to_frames(apply.normalise(synth.mixture(seed, (400 + (nfr - 1) * 160) / 16000.0)))
        lm = O.logmag_phase(O.stft(mix))[0].astype(np.float32)
        assert lm.shape[0] == nfr, lm.shape
        lms.append(lm)
    return lms, ctx


_pool_cache = [None, None]


def pool_reference(kind):
    """(W, lms, ctx, emb_in, [ClipRef f64 per pool clip], [ClipRef f32], t64, t32 of layer_checks.reference) on the
    `synthetic7` weights: clips 0..2 are slices of layer_checks' batch reference (computed once, shared with the layer
    tests), the three extra clips -- four frames -- are computed here."""
    import torch
    import layer_checks as L
    from oracle.torch_ref import TorchRef
    if _pool_cache[0] == kind:
        return _pool_cache[1]
    W, lms3, ctx, emb_in, t64, t32 = L.reference(kind, "synthetic7")
    lms, _ = pool_features()
    refs = {}
    for dtype, t in ((torch.float64, t64), (torch.float32, t32)):
        emb = torch.from_numpy(np.asarray(emb_in, dtype=np.float32)).to(dtype)
        ref = TorchRef(W, kind, dtype)
        clips = []
        for i, nfr in enumerate(POOL_FRAMES):
            c = ClipRef()
            if i < 3:
                sl = slice(L.FOFF[i], L.FOFF[i + 1])
                c.acts = {idx: t.acts[idx][sl] for idx in L.STACK_IDX}
                c.logits, c.denoised = t.logits[sl], t.denoised[sl]
            else:
                a, b = POOL_PAIRS[i]
                c.acts = {}
                with torch.no_grad():
                    win = ref.windows(torch.from_numpy(lms[i]).to(dtype))
                    c.logits, c.denoised = ref.mask_net(win, emb[a][None].expand(nfr, -1), emb[b][None].expand(nfr, -1), c.acts)
            clips.append(c)
        refs[dtype] = clips
    _pool_cache[:] = [kind, (W, lms, ctx, emb_in, refs[torch.float64], refs[torch.float32], t64, t32)]
    return _pool_cache[1]


# ---- geometries --------------------------------------------------------------------------------------------------
# An entry of the table: order (pool clip indices, in batch order), fpc (option frames_per_chunk), frame0 / nframes (the
# range the debug tap fetches: its passes are counted from frame0; the logits are always taken of the whole batch in
# passes of fpc from frame 0), tensors (the stored tensors to compare besides the heads: those whose launches the entry
# was chosen for), name (a regression case's name, else "")
def entry_frames(e):
    """(clip instance of every frame of the batch, its clip's length, offsets of the clip instances)."""
    lens = [POOL_FRAMES[i] for i in e["order"]]
    foff = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    cid = np.repeat(np.arange(len(lens)), lens)
    clen = np.repeat(lens, lens)
    return cid, clen, foff


def tap_passes(e):
    """[(first frame, frames)] of the debug tap's passes."""
    wf = min(e["fpc"], e["nframes"])
    return [(g0, min(wf, e["frame0"] + e["nframes"] - g0)) for g0 in range(e["frame0"], e["frame0"] + e["nframes"], wf)]


def head_passes(e):
    total = int(entry_frames(e)[2][-1])
    wf = min(e["fpc"], total)
    return [(g0, min(wf, total - g0)) for g0 in range(0, total, wf)]


def entry_cover(cfg, e):
    """{(launch kind, bucket)} the entry hits in configuration cfg, over every row_split value that changes a launch: the
    tap's passes for the launches that write one of the entry's `tensors`, the whole-batch passes for the head's dense
    layer."""
    cid, clen, foff = entry_frames(e)
    hit = set()
    for rs in row_splits(cfg):
        for heads, plist in ((False, tap_passes(e)), (True, head_passes(e))):
            for g0, n in plist:
                edges = set()
                if g0 > 0 and cid[g0] == cid[g0 - 1]: edges.add("pass starts in a clip")
                if g0 + n < len(cid) and cid[g0 + n] == cid[g0 + n - 1]: edges.add("pass ends in a clip")
                if not heads and e["frame0"] > 0: edges.add("frame0>0")
                for l in stack_launches(cfg, n, rs):
                    if (l.tensor == HEADS_TENSOR) != heads or not (heads or l.tensor in e["tensors"]):
                        continue
                    for b in size_buckets(l) | clip_buckets(l, cid[g0:g0 + n], clen[g0:g0 + n]) | edges:
                        hit.add((kind_of(l), b))
    return hit


def universe(cfg):
    """{(launch kind, bucket): None if some pass of 1 .. MAX_PASS frames can hit it, else the reason it cannot}, and
    {launch kind: a Launch of it}."""
    kinds, reach = {}, set()
    for rs in row_splits(cfg):
        for n in range(1, MAX_PASS + 1):
            for l in stack_launches(cfg, n, rs):
                k = kind_of(l)
                kinds.setdefault(k, l)
                for b in size_buckets(l):
                    reach.add((k, b))
    out = {}
    for k, l in kinds.items():
        for b in applicable(l):
            ok = clip_reachable(l, b) if b in CLIP_BUCKETS else (k, b) in reach
            out[(k, b)] = None if ok else unreachable_reason(l, b)
        for b in PASS_BUCKETS:
            heads0 = l.tensor == HEADS_TENSOR and b == "frame0>0"
            out[(k, b)] = "nhans_mask_net always starts at frame 0; the tap has no head rows" if heads0 else None
    return out, kinds


def unreachable_reason(l, b):
    """Why no pass of 1 .. MAX_PASS frames puts a launch of l's kind into bucket b (l: the kind's launch of one pass)."""
    if b == "4clips":
        return "a %d-pixel tile touches at most %d frames of %d pixels" % (l.tile, max_frames_in_tile(l), l.px)
    if b == "end+1f":
        return "a frame is %d pixels: a partial last tile of %d lies inside the last frame" % (l.px, l.tile)
    if b == "capped":
        return "the grid stays below its cap for passes of up to %d frames" % MAX_PASS
    if b == "grid<8":
        return "one frame is already eight or more workgroups"
    if b.startswith("grid"):
        mult = l.grid // (l.M // l.px) if l.per_frame else l.grid // -(-l.M // l.tile)
        return "the grid is a multiple of %d (%s): never %s mod 8 in a pass of up to %d frames" % (
            mult, "workgroups per frame" if l.per_frame else "channel tiles per pixel tile", b[-1], MAX_PASS)
    if b == "M<tile":
        return "one frame is %d pixels, no less than the %d-pixel tile" % (l.px, l.tile)
    return "M = n x %d: every residue mod %d is a multiple of %d, and the window holds none" % (l.px, l.tile, int(np.gcd(l.px, l.tile)))


def load_table():
    with open(TABLE_PATH) as f:
        return json.load(f)


# ---- the tower ---------------------------------------------------------------------------------------------------
TOWER_MAX = 9


def tower_cases(cfg):
    """(images, contexts_per_chunk) for batches of 1 .. 9 images: a greedy cover of the size and grid buckets of the
    tower's launches that passes of 1 .. 9 images can hit at all (computed here: the search is a few hundred cases)."""
    def cover(n, cpc):
        hit = set()
        for g0 in range(0, n, cpc):
            for l in tower_launches(cfg, min(cpc, n - g0)):
                hit |= {(kind_of(l), b) for b in size_buckets(l)}
        return hit
    cands = [(n, cpc) for n in range(1, TOWER_MAX + 1) for cpc in range(1, n + 1)]
    todo = set().union(*(cover(*c) for c in cands))
    total, chosen = set(todo), []
    while todo:
        best = max(cands, key=lambda c: (len(cover(*c) & todo), -c[0]))
        chosen.append(best)
        todo -= cover(*best)
    return chosen, total


# ---- the comparison ----------------------------------------------------------------------------------------------
def locate(cfg, e, row_split, tensor, frame, h, w, heads=False):
    """The launches that write element (frame of the batch, h, w) of stored tensor `tensor` (HEADS_TENSOR: row `frame` of
    the logits / denoised rows) under entry e: [(Launch, tile index, row within the tile, first frame of the pass)]."""
    plist = head_passes(e) if heads else tap_passes(e)
    out = []
    for g0, n in plist:
        if not g0 <= frame < g0 + n:
            continue
        for l in stack_launches(cfg, n, row_split):
            if l.tensor != tensor or not (l.oh0 <= h < l.oh0 + l.rows):
                continue
            m = (frame - g0) * l.px + (h - l.oh0) * l.wo + w
            if l.per_frame:
                out.append((l, None, None, g0))
            else:
                out.append((l, m // l.tile, m % l.tile, g0))
    return out


def describe_difference(cfg, e, row_split, tensor, got, want, frames, heads=False, label=""):
    """None if got and want (arrays of one shape: [frames, H, W, C] of a stored tensor or [frames, 201] head rows, numpy or
    torch, host or device) hold the same bits; else a message that names the first differing element -- tensor, kernel, M,
    tile, tile index, row within the tile, clip, frame, pixel, channel -- and counts the differing ones.  frames: the
    batch frame of every row of the arrays."""
    import torch
    g, t = torch.as_tensor(got), torch.as_tensor(want)
    assert g.shape == t.shape and g.dtype == t.dtype == torch.float32, (g.shape, t.shape, g.dtype, t.dtype)
    ne = g.contiguous().view(torch.int32) != t.contiguous().view(torch.int32)
    count = int(ne.sum())
    if not count:
        return None
    shape = tuple(g.shape) if g.ndim == 4 else (g.shape[0], 1, 1, g.shape[1])
    flat = int(torch.nonzero(ne.reshape(-1))[0])
    i, rem = divmod(flat, shape[1] * shape[2] * shape[3])
    h, rem = divmod(rem, shape[2] * shape[3])
    w, c = divmod(rem, shape[3])
    frame = int(frames[i])
    cid, clen, foff = entry_frames(e)
    ci = int(cid[frame])
    name = "logits / denoised rows" if heads else __import__("layer_checks").NAMES[tensor]
    where = []
    for l, ti, row, g0 in locate(cfg, e, row_split, HEADS_TENSOR if heads else tensor, frame, 0 if heads else h, 0 if heads else w, heads):
        if l.per_frame:
            where.append("%s %s (tiles each frame alone, grid %d, pass of %d frames from %d)" % (l.conv, l.kernel, l.grid, l.M // l.px, g0))
        else:
            ntile = -(-l.M // l.tile)
            where.append("%s %s%s M %d tile %d: tile %d of %d%s, row %d of it (pass of %d frames from %d)" % (
                l.conv, l.kernel, " " + l.cls if l.cls else "", l.M, l.tile, ti, ntile,
                " (the partial last tile, %d rows)" % (l.M % l.tile) if ti == ntile - 1 and l.M % l.tile else "", row, l.M // l.px, g0))
    return ("%stensor %d (%s), row_split %d: %d of %d elements differ; first at frame %d (frame %d of clip instance %d = pool clip %d, "
            "%d frames), pixel (h %d, w %d), channel %d: got %.9g want %.9g; written by %s" % (
                label + ": " if label else "", tensor, name, row_split, count, g.numel(), frame, frame - int(foff[ci]), ci,
                e["order"][ci], int(clen[frame]), h, w, c, float(g.reshape(-1)[flat]), float(t.reshape(-1)[flat]),
                "; ".join(where) or "no launch of the restatement"))
