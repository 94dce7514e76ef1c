"""Stack and tower tensors, bit for bit, at every conv tile edge.

The contract: the bits of a frame do not depend on where the frame sits in a batch or a pass.  So per arithmetic mode
(tests/geometry_checks.py: MODES)

  anchor      every clip of a pool of six (11, 1, 9, 1, 1 and 2 frames, no two with the same conditioning pair) is run ALONE:
              stored tensors 8 .. 24, logits and denoised rows, held to float64 at the bar of the layer tests
              (layer_checks.check_tensor / check_head, BAR unchanged);
  geometries  every entry of the committed table (tests/golden/geometry_table.json; tests/test_geometry_checks_host.py
              shows that it hits a full last tile, one of one or two rows, one that ends at an MFMA block, a wave or half
              the tile, a launch below one tile, grids the XCD remap does not divide evenly, tiles with rows of four
              clips, the end of a clip and a one-frame clip in a partial last tile, passes that start and end inside a
              clip, a tap from frame0 > 0 -- for every launch kind of the mode that can be brought there): logits,
              denoised rows and the stored tensors the entry was chosen for == the clips alone, bit for bit, compared on
              the device.  In f16x3 again with row_split 0 and 2, epilogue_wide 0 and consumer_interleave 0 and 2, which
              are bit-identical by contract;
  profile     one chunked geometry per mode with `profile` on: the kernel names and the calls per name are exactly what
              the restatement of the launches predicts, for every row_split value -- the table of tiles the buckets are
              computed from cannot go stale unnoticed.

The tower: batches of 1 .. 9 context images with contexts_per_chunk from the same bucket rule, tensors 0 .. 7 and the
embeddings == each image alone, with split_k 1 and 0, in f16x3 and f32.

Every case prints its measured time."""
import time

import numpy as np
import pytest
import torch

import nhans_amd  # noqa: F401
from nhans_amd import engine
import geometry_checks as G
import layer_checks as L

pytestmark = pytest.mark.gpu

DEFAULTS = {"winograd": 1, "conv_variant": -1, "winograd_f32_tensors": 1, "frames_per_chunk": 3776, "contexts_per_chunk": 64,
            "split_k": 1, "row_split": 1, "epilogue_wide": 1, "consumer_interleave": 1, "profile": 0}
# the settings that leave every bit alone (f16x3); the first is what the clips alone were fetched with
SETTINGS = [{}, {"row_split": 0}, {"row_split": 2}, {"epilogue_wide": 0}, {"consumer_interleave": 0}, {"consumer_interleave": 2}]


def _configure(eng, cfg, extra=None):
    eng.set_precision(cfg.prec)
    for k, v in DEFAULTS.items():
        eng.set_option(k, dict(cfg.options, **(extra or {})).get(k, v))


def _same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def _pieces(e, first, count):
    """[(pool clip, first frame within the clip, frames)] that make frames [first, first + count) of entry e's batch."""
    cid, clen, foff = G.entry_frames(e)
    out, g = [], first
    while g < first + count:
        ci = int(cid[g])
        end = min(int(foff[ci + 1]), first + count)
        out.append((e["order"][ci], g - int(foff[ci]), end - g))
        g = end
    return out


def _expected(alone, key, pieces):
    return torch.cat([alone[c][key][a:a + n] for c, a, n in pieces])


@pytest.mark.parametrize("mode", [m[0] for m in G.MODES])
def test_every_geometry_gives_the_bits_of_the_clip_alone(lib_built, mode):
    _, kind, config = next(m for m in G.MODES if m[0] == mode)
    cfg = G.CONFIGS[config]
    t_start = time.time()
    W, lms, ctx, emb_in, c64, c32, _, _ = G.pool_reference(kind)
    t_ref = time.time() - t_start
    emb = np.asarray(emb_in, dtype=np.float32)
    eng = engine.Engine(kind, W, precision="f16x3")
    failures, rows = [], []
    try:
        lm_dev = [torch.from_numpy(lm).cuda() for lm in lms]
        ea_pool = torch.from_numpy(emb[[a for a, _ in G.POOL_PAIRS]]).cuda()
        eb_pool = torch.from_numpy(emb[[b for _, b in G.POOL_PAIRS]]).cuda()

        # ---- anchor: every pool clip alone, against float64 at the layer tests' bar
        t0 = time.time()
        _configure(eng, cfg)
        alone = []
        for i, nfr in enumerate(G.POOL_FRAMES):
            a = {idx: eng.activation(idx, lm_dev[i], [0, nfr], ea_pool[i:i + 1], eb_pool[i:i + 1], 0, nfr) for idx in L.STACK_IDX}
            a["logits"], a["denoised"] = eng.mask_net(lm_dev[i], [0, nfr], ea_pool[i:i + 1], eb_pool[i:i + 1])
            alone.append(a)
        assert eng.take_status() == 0
        t64, t32 = L.Taps(), L.Taps()
        for t, refs in ((t64, c64), (t32, c32)):
            t.acts = {idx: torch.cat([r.acts[idx] for r in refs]) for idx in L.STACK_IDX}
            t.logits, t.denoised = torch.cat([r.logits for r in refs]), torch.cat([r.denoised for r in refs])
        pool_off = [0] + list(np.cumsum(G.POOL_FRAMES))
        for idx in L.STACK_IDX:
            v = L.check_tensor(idx, torch.cat([a[idx] for a in alone]), t64, t32, cfg.prec, mode + ", clips alone")
            rows.append("%-32s %s" % (mode, v.row()))
            if not v.ok:
                failures.append(v.message)
        for name, r64, r32 in (("logits", t64.logits, t32.logits), ("denoised", t64.denoised, t32.denoised)):
            v = L.check_head(name, torch.cat([a[name] for a in alone]), r64, r32, cfg.prec, mode + ", clips alone", foff=pool_off)
            rows.append("%-32s %s" % (mode, v.row()))
            if not v.ok:
                failures.append(v.message)
        t_anchor = time.time() - t0

        # ---- every geometry of the table, under every setting that must not move a bit
        t0 = time.time()
        settings = SETTINGS if cfg.prec == "f16x3" else SETTINGS[:1]
        entries = G.load_table()[config]["entries"]
        fetches = frames = 0
        for ei, e in enumerate(entries):
            lm = torch.cat([lm_dev[c] for c in e["order"]])
            foff = [int(v) for v in G.entry_frames(e)[2]]
            sel = torch.tensor(e["order"], device=lm.device)
            ea, eb = ea_pool[sel], eb_pool[sel]
            whole, part = _pieces(e, 0, foff[-1]), _pieces(e, e["frame0"], e["nframes"])
            want = {"logits": _expected(alone, "logits", whole), "denoised": _expected(alone, "denoised", whole)}
            for idx in e["tensors"]:
                want[idx] = _expected(alone, idx, part)
            for extra in settings:
                _configure(eng, cfg, dict(extra, frames_per_chunk=e["fpc"]))
                rs = extra.get("row_split", 1)
                label = "%s, entry %d%s (%d frames in %d clips, fpc %d, tap [%d, %d)), %s" % (
                    mode, ei, " " + e["name"] if e["name"] else "", foff[-1], len(e["order"]), e["fpc"], e["frame0"],
                    e["frame0"] + e["nframes"], extra or "default settings")
                lg, den = eng.mask_net(lm, foff, ea, eb)
                for name, got in (("logits", lg), ("denoised", den)):
                    if not _same_bits(got, want[name]):
                        failures.append(name + ": " + G.describe_difference(cfg, e, rs, G.HEADS_TENSOR, got, want[name], np.arange(foff[-1]), True, label))
                for idx in e["tensors"]:
                    got = eng.activation(idx, lm, foff, ea, eb, e["frame0"], e["nframes"])
                    if not _same_bits(got, want[idx]):
                        failures.append(G.describe_difference(cfg, e, rs, idx, got, want[idx], np.arange(e["frame0"], e["frame0"] + e["nframes"]), False, label))
                    del got
                st = eng.take_status()
                if st:
                    failures.append("%s: status %d" % (label, st))
                fetches += 1 + len(e["tensors"])
                frames += foff[-1] + len(e["tensors"]) * e["nframes"]
            del want
            if len(failures) > 20:
                break
        torch.cuda.synchronize()
        t_geo = time.time() - t0

        # ---- the restatement against the launches that run: one chunked geometry, every row_split value
        t0 = time.time()
        e = next(e for e in entries if len(G.head_passes(e)) >= 2)
        lm = torch.cat([lm_dev[c] for c in e["order"]])
        foff = [int(v) for v in G.entry_frames(e)[2]]
        sel = torch.tensor(e["order"], device=lm.device)
        for rs in (0, 1, 2):
            _configure(eng, cfg, {"row_split": rs, "frames_per_chunk": e["fpc"], "profile": 1})
            eng.profile_reset()
            eng.mask_net(lm, foff, ea_pool[sel], eb_pool[sel])
            got = {k: v["calls"] for k, v in eng.profile().items()}
            predicted = G.profile_calls(cfg, [n for _, n in G.head_passes(e)], rs if rs in G.row_splits(cfg) else 1)
            if got != predicted:
                failures.append("%s, row_split %d, passes %s: the profile shows %s, the restatement predicts %s" % (
                    mode, rs, [n for _, n in G.head_passes(e)], sorted(got.items()), sorted(predicted.items())))
        _configure(eng, cfg)
        t_prof = time.time() - t0
    finally:
        eng.close()
    print("\n%s: CPU references %.1f s; on the device: anchor %.2f s, %d geometries x %d settings (%d fetches, %d frames) %.2f s, "
          "profile %.2f s; whole case %.1f s" % (mode, t_ref, t_anchor, len(entries), len(settings), fetches, frames, t_geo, t_prof,
                                                 time.time() - t_start))
    print("\n".join(rows))
    assert not failures, "%d failures:\n%s" % (len(failures), "\n".join(failures[:12]))


def test_tower_images_give_the_bits_of_the_image_alone(lib_built):
    t_start = time.time()
    _, ctx = L.features()
    eng = engine.Engine("denoiser", L.WEIGHTS["synthetic7"]("denoiser"), precision="f16x3")
    failures, lines = [], []
    try:
        img = torch.from_numpy(ctx).cuda()
        for config in ("f16x3", "f32"):
            cfg = G.CONFIGS[config]
            t0 = time.time()
            _configure(eng, cfg)
            alone = [dict({idx: eng.tower_activation(idx, img[i:i + 1]) for idx in L.TOWER_IDX}, emb=eng.embed(img[i:i + 1]))
                     for i in range(L.N_CTX)]
            assert eng.take_status() == 0
            cases, total = G.tower_cases(cfg)
            for n, cpc in cases:
                which = [i % L.N_CTX for i in range(n)]
                batch = img[which]
                for split_k in (1, 0):
                    _configure(eng, cfg, {"contexts_per_chunk": cpc, "split_k": split_k})
                    for key in L.TOWER_IDX + ["emb"]:
                        got = eng.embed(batch) if key == "emb" else eng.tower_activation(key, batch)
                        want = torch.cat([alone[i][key] for i in which])
                        if not _same_bits(got, want):
                            ne = (got.view(torch.int32) != want.view(torch.int32))
                            first = torch.nonzero(ne.reshape(n, -1).any(dim=1))[0].item()
                            written = [G.kind_of(l) + " M %d tile %d grid %d" % (l.M, l.tile, l.grid)
                                       for l in G.tower_launches(cfg, min(cpc, n - first // cpc * cpc)) if l.tensor == key]
                            failures.append("%s, %d images in passes of %d, split_k %d: %s differs from the images alone in %d elements, "
                                            "first in image %d (context %d, image %d of its pass); written by %s" % (
                                                config, n, cpc, split_k, "embeddings" if key == "emb" else "tensor %d (%s)" % (key, L.NAMES[key]),
                                                int(ne.sum()), first, which[first], first % cpc, "; ".join(written) or "avgpool"))
                    st = eng.take_status()
                    if st:
                        failures.append("%s, %d images in passes of %d, split_k %d: status %d" % (config, n, cpc, split_k, st))
            torch.cuda.synchronize()
            lines.append("tower %s: %d (images, contexts_per_chunk) cases %s for %d (launch kind, bucket) pairs, x split_k 1 / 0: %.2f s" % (
                config, len(cases), cases, len(total), time.time() - t0))
        _configure(eng, G.CONFIGS["f16x3"])
    finally:
        eng.close()
    print("\n" + "\n".join(lines) + "\nwhole case %.1f s" % (time.time() - t_start))
    assert not failures, "%d failures:\n%s" % (len(failures), "\n".join(failures[:12]))
