// nhans_bss_eval (include/nhans_hip.h): the run table, the groups and the launches of bsseval.hip.  What the call refuses
// needs no device and is refused before the context is looked at.
//   Groups.  The factor of a clip's Gram matrix takes M^2 doubles of the workspace (M = J L: 8 MiB at J = 2, L = 512; the
// target-only filter C0 is solved from its leading block, so there is no second matrix).  The clips of a call are worked
// in groups of consecutive clips whose factors together stay within the context's bss_group_bytes (2 GiB: 256 clips at
// full size; a group holds at least one clip), one plan and one launch sequence per group.  Every kernel works a clip from
// its own run alone, so the grouping changes no bit of any record.
#include "host_internal.h"

extern "C" {

int nhans_bss_eval(nhans_ctx* c, const float* est, const int64_t* eoff, const float* const* src, const int64_t* const* soff, int nsrc,
                   int nclips, int filt_len, double* out, double* filters_out, void* stream) {
    const std::string fn = "nhans_bss_eval";
    if (nclips < 0) return fail(NHANS_EINVAL, fn + ": negative clip count");
    if (nsrc != 1 && nsrc != 2) return fail(NHANS_EINVAL, fn + ": " + std::to_string(nsrc) + " sources (1: the target, or 2: target and interferer)");
    if (filt_len < 1 || filt_len > kBssMaxL)
        return fail(NHANS_EINVAL, fn + ": filter length " + std::to_string(filt_len) + " (1 ... " + std::to_string(kBssMaxL) + ")");
    if (nclips > 0 && (!eoff || !src || !soff || !out))
        return fail(NHANS_EINVAL, fn + ": null offsets, null source table or null output with " + std::to_string(nclips) + " clips to score");
    for (int j = 0; nclips > 0 && j < nsrc; ++j)
        if (!soff[j]) return fail(NHANS_EINVAL, fn + ": null offsets of source " + std::to_string(j) + " with " + std::to_string(nclips) + " clips to score");
    int rc = offsets_check(fn, "estimate", eoff, nclips); if (rc) return rc;
    for (int j = 0; nclips > 0 && j < nsrc; ++j) {
        rc = offsets_check(fn, j ? "interferer" : "target", soff[j], nclips); if (rc) return rc;
    }
    const int L = filt_len, J = nsrc, M = J * L, NI = J == 2 ? 6 : 2;
    std::vector<BssRun> runs((size_t)nclips);
    for (int i = 0; i < nclips; ++i) {
        int64_t n = eoff[i + 1] - eoff[i];
        for (int j = 0; j < J; ++j) n = std::min(n, soff[j][i + 1] - soff[j][i]);
        if (n > kMaxResampleClip)
            return fail(NHANS_EINVAL, fn + ": clip " + std::to_string(i) + " has " + std::to_string(n) + " samples (0 ... 2^31 - 1)");
        if (n > 0 && (!est || !src[0] || (J == 2 && !src[1]))) return null_clip(fn, i, n);
        const long long T = n + L - 1;
        runs[i] = {n > 0 ? est + eoff[i] : nullptr, n > 0 ? src[0] + soff[0][i] : nullptr, n > 0 && J == 2 ? src[1] + soff[1][i] : nullptr,
                   (long long)n, 0, (n + kBssCorrTile - 1) / kBssCorrTile, 0, (T + kBssProjTile - 1) / kBssProjTile};
    }
    return ctx_call(c, stream, [&](hipStream_t s) -> int {
        const size_t per_clip = (size_t)M * M * sizeof(double);
        for (int g0 = 0; g0 < nclips;) {
            // the group: clips [g0, g1)
            int g1 = g0;
            long long ct = 0, pt = 0, ns = 0;
            while (g1 < nclips && (g1 == g0 || ((size_t)(g1 - g0 + 1) * per_clip <= c->bss_group_bytes &&
                                                ct + runs[g1].ctiles <= 0x7fffffffLL && pt + runs[g1].ptiles <= 0x7fffffffLL))) {
                runs[g1].ctile0 = ct; runs[g1].ptile0 = pt;
                ct += runs[g1].ctiles; pt += runs[g1].ptiles; ns += runs[g1].n;
                ++g1;
            }
            const int g = g1 - g0;
            WsPlan p;
            BssRun* runs_dev; double *part, *lag, *G, *sol, *epart; int* flag;
            p.add(&runs_dev, (size_t)g);
            p.add(&part, (size_t)ct * NI * L);
            p.add(&lag, (size_t)g * NI * L);
            p.add(&G, (size_t)g * M * M);
            p.add(&sol, (size_t)g * (M + L));
            p.add(&flag, (size_t)g);
            p.add(&epart, (size_t)pt * 6);
            rc = ws_commit(c, p); if (rc) return rc;
            rc = h2d(c, runs_dev, runs.data() + g0, (size_t)g * sizeof(BssRun), s); if (rc) return rc;
            const double C = (double)g, N = (double)ns, CT = (double)ct, PT = (double)pt, Md = (double)M, Ld = (double)L, NIL = (double)NI * L;
            const double TT = N + C * (Ld - 1.0);       // samples of the projections
            {   // per sample and lag: NI fused multiply-adds
                Prof pr(c, s, "bss_corr");
                launch_bss_corr("bss_corr", runs_dev, g, ct, L, J, part, s);
                pr.done(2.0 * NIL * N, 4.0 * (J + 1) * (N + CT * (Ld - 1.0)) + 8.0 * CT * NIL);
            }
            {
                Prof pr(c, s, "bss_reduce");
                launch_bss_reduce("bss_reduce", runs_dev, g, L, J, part, lag, s);
                pr.done(CT * NIL, 8.0 * CT * NIL + 8.0 * C * NIL);
            }
            {
                Prof pr(c, s, "bss_gram");
                launch_bss_gram("bss_gram", g, L, J, lag, G, s);
                pr.done(0.0, 8.0 * C * (NIL + Md * (Md + 1.0) / 2.0));
            }
            {   // M^3 / 3 for the factor, M^2 for each of the solves; the trailing matrix is read and written once per panel
                Prof pr(c, s, "bss_chol");
                launch_bss_chol("bss_chol", g, L, J, lag, G, sol, filters_out ? filters_out + (size_t)g0 * (M + L) : nullptr, flag, s);
                pr.done(C * (Md * Md * Md / 3.0 + 2.0 * Md * Md + (J == 2 ? Ld * Ld : 0.0)),
                        C * (16.0 * Md * Md * Md / (6.0 * kBssPanel) + 8.0 * Md * Md + 8.0 * (J == 2 ? 1.5 : 1.0) * Md * Md / 2.0));
            }
            {   // per sample: (J + 1) L fused multiply-adds and the six squares
                Prof pr(c, s, "bss_project");
                launch_bss_project("bss_project", runs_dev, g, pt, L, J, sol, flag, epart, s);
                pr.done(TT * (2.0 * (J + 1) * Ld + 16.0), 4.0 * J * (TT + PT * (Ld - 1.0)) + 4.0 * N + 8.0 * PT * ((Md + Ld) + 6.0));
            }
            {
                Prof pr(c, s, "bss_finish");
                launch_bss_finish("bss_finish", runs_dev, g, L, J, flag, epart, out + (size_t)g0 * kBssFields, s);
                pr.done(6.0 * PT + 40.0 * C, 48.0 * PT + 8.0 * kBssFields * C);
            }
            g0 = g1;
        }
        return NHANS_OK;
    });
}

}  // extern "C"
