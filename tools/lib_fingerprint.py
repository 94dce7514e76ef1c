"""Dev tool: a fingerprint of what the library under $NHANS_LIB computes -- sha256 of the logits of the golden exp2 features
(f16x3 with the Winograd form on and off, f32) and of a three-clip ragged end-to-end batch; then one sha256 per scoring
family (score, STOI, quality, BSS Eval, align) over the raw bytes of its records and of every optional output, on a seeded
batch of the smallest clips that reach each tile edge and the run search, no clip 16-byte aligned.  Two builds that are
meant to differ in speed only (tools/ab_variant_libs.sh, tools/ab_libs.sh) must print the same lines.
    NHANS_LIB=build_ab/variants/libnhans_X.so python tools/lib_fingerprint.py"""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nhans_amd  # noqa: E402,F401
from nhans_amd import apply, context, engine, hip, score, synth  # noqa: E402
import stoi_checks  # noqa: E402

PAD = 3         # floats before the first clip of every flat buffer: no clip begins on a 16-byte boundary


def _digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().cpu().numpy().tobytes())
    return h.hexdigest()[:16]


def _pairs(rng, lengths, noise=0.05):
    """-> (estimates, targets): seeded float32 clips, estimate i = target i + noise"""
    tgt = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in lengths]
    return [(t + noise * 0.1 * rng.standard_normal(len(t))).astype(np.float32) for t in tgt], tgt


def _flat(clips):
    """-> (device tensor: PAD floats, then the clips; the clips' offsets in it)"""
    off = [PAD + o for o in context.offsets(len(c) for c in clips)]
    return torch.from_numpy(np.concatenate([np.zeros(PAD, np.float32)] + list(clips))).cuda(), off


def scoring(eng):
    """One line per scoring family."""
    rng = np.random.default_rng(20240611)
    out = []
    # score: the tile of 2560, the segment of 80, the frame of 400, an empty clip between others
    es, ts = _pairs(rng, (1, 0, 399, 400, 2559, 2560, 2561, 5121))
    (e, eo), (t, to) = _flat(es), _flat(ts)
    rec, fr = eng.score_device(e, eo, t, to, per_frame=True)
    foff = context.offsets(int(eng.lib.nhans_num_frames(len(x))) for x in es)
    rows = [torch.from_numpy(np.concatenate([np.zeros(PAD, np.float32), rng.standard_normal(foff[-1] * 201).astype(np.float32)])).cuda()[PAD:]
            .view(foff[-1], 201) for _ in range(2)]
    rrec, fr = eng.score_rows(rows[0], rows[1], foff, per_frame=True, frames_out=fr)
    out.append("score wave + rows  %s" % _digest(rec, rrec, fr))
    # STOI at 10 kHz: 0, 0, 1 and 17 segments, a clip whose kept frames are every second one; one clip through 16 kHz
    es, ts = _pairs(rng, (256, 4096, 4097, 6145))
    ce, ct = stoi_checks.compaction_clip("every_second")
    (e, eo), (t, to) = _flat(es + [ce]), _flat(ts + [ct])
    rec, seg, _ = eng.stoi_device(e, eo, t, to, rate=score.STOI_RATE, per_segment=True)
    es, ts = _pairs(rng, (9000,))
    (e, eo), (t, to) = _flat(es), _flat(ts)
    rec16, seg16, _ = eng.stoi_device(e, eo, t, to, rate=16000, per_segment=True)
    out.append("stoi               %s" % _digest(rec, seg, rec16, seg16))
    # quality: 0, 0, 1, 7, 8 and 15 frames (LPC tile 7, band tile 2), a silent stretch in one target, default bands and K = 1
    es, ts = _pairs(rng, (0, 479, 480, 1200, 1320, 2160))
    ts[5][600:1200] = 0.0
    (e, eo), (t, to) = _flat(es), _flat(ts)
    rec, fr, foff = eng.quality_device(e, eo, t, to, per_frame=True)
    one = np.linspace(0.0, 1.0, score.QUALITY_BINS)[None, :]
    rec1, fr1, _ = eng.quality_device(e, eo, t, to, per_frame=True, bands=one)
    lpc = torch.empty((max(foff[-1], 1), hip.QUALITY_LPC_FIELDS), dtype=torch.float64, device=e.device)
    hip.check(eng.lib.nhans_quality_lpc(eng.handle, hip.ptr(e), hip.i64_array(eo), hip.ptr(t), hip.i64_array(to), len(es), hip.ptr(lpc),
                                        eng._stream()))
    out.append("quality            %s" % _digest(rec, fr, rec1, fr1, lpc[:foff[-1]]))
    # BSS Eval: the correlation tile of 2048 and the projection tile of 1024, one and two sources, a singular clip
    es, ts = _pairs(rng, (0, 1, 1023, 1024, 1025, 2049, 1500))
    xs = [(0.1 * rng.standard_normal(len(x))).astype(np.float32) for x in ts]
    xs[6][:] = 0.0
    (e, eo), (t, to), (x, xo) = _flat(es), _flat(ts), _flat(xs)
    got = []
    for L, J in ((16, 1), (16, 2), (300, 2)):
        got.extend(eng.bss_eval_device(e, eo, [(t, to), (x, xo)][:J], filt_len=L, filters=True))
    out.append("bss_eval           %s" % _digest(*got))
    # align: one and two lag blocks, the sample tile of 2048, empty pairs; the ragged cut
    lens = ((0, 0), (1, 1), (2049, 2048), (3000, 4097))
    es = [(0.1 * rng.standard_normal(ne)).astype(np.float32) for ne, _ in lens]
    ts = [(0.1 * rng.standard_normal(nt)).astype(np.float32) for _, nt in lens]
    (e, eo), (t, to) = _flat(es), _flat(ts)
    got = []
    for D in (0, 5, 1100):
        got.extend(eng.align_device(e, eo, t, to, max_lag=D, corr=True))
    ce, ct, _ = eng.align_cut_device(e, eo, t, to, [0, 0, 7, -7])
    out.append("align + cut        %s" % _digest(*got, ce, ct))
    return out


def main():
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "case_exp2.npz")))
    eng = engine.Engine("denoiser", precision="f16x3")
    lm = torch.from_numpy(g["logmag"]).cuda()
    ea = torch.from_numpy(g["emb_a"][None]).cuda()
    eb = torch.from_numpy(g["emb_b"][None]).cuda()
    out = []
    for prec, wino in (("f16x3", 1), ("f16x3", 0), ("f32", 1)):
        eng.set_precision(prec)
        eng.set_option("winograd", wino)
        lg = eng.mask_net(lm, [0, 308], ea, eb)[0].cpu().numpy()
        out.append("%s winograd=%d logits %s (vs golden %.2e)" % (prec, wino, hashlib.sha256(lg.tobytes()).hexdigest()[:16], np.abs(lg - g["logits"]).max()))
    eng.set_precision("f16x3")
    eng.set_option("winograd", 1)
    mixes = [apply.trim_to_frames(apply.normalise(synth.mixture(900 + i, s))) for i, s in enumerate((1.3, 0.4, 10.0))]
    ca = [apply.normalise(synth.silent()) for _ in mixes]
    cb = [apply.normalise(synth.noise_context(900 + i)) for i in range(3)]
    res = eng.enhance(mixes, ca, cb, want_mixed=True, taps=True)
    h = hashlib.sha256()
    for k in ("denoised_wav", "mixed_wav"):
        for w in res[k]:
            h.update(w.tobytes())
    h.update(res["logits"].tobytes())
    out.append("3-clip batch end to end %s" % h.hexdigest()[:16])
    out.extend(scoring(eng))
    print(os.environ.get("NHANS_LIB", "default library"))
    for l in out:
        print("  " + l)


if __name__ == "__main__":
    main()
