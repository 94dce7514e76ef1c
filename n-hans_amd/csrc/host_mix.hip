// nhans_mix / nhans_mix_snr_factor (include/nhans_hip.h): the chain and job tables and the three launches of mix.hip.  What
// the call refuses needs no device and is refused before the context is looked at.
#include "host_internal.h"

extern "C" {

int nhans_mix_snr_factor(double snr_db, double* factor_out) {
    if (!factor_out) return fail(NHANS_EINVAL, "nhans_mix_snr_factor: null output");
    volatile double ten = 10.0;     // (the C library's pow itself: a constant base invites the compiler to call another function)
    *factor_out = pow(ten, -snr_db / 10.0);
    return NHANS_OK;
}

int nhans_mix(nhans_ctx* c, const float* speech, const int64_t* soff, int nspeech, const float* noise, const int64_t* noff,
              int nnoise, const int* si, const int* ki, const int* di, const double* snr_keep, const double* snr_drop, int njobs,
              float* mixture, float* target, float* keep, float* drop, const int64_t* ooff, double* records, void* stream) {
    const std::string fn = "nhans_mix";
    if (njobs < 0) return fail(NHANS_EINVAL, fn + ": negative job count");
    if (nspeech < 0 || nnoise < 0) return fail(NHANS_EINVAL, fn + ": negative clip count");
    if (njobs > 0 && (!speech || !soff || !noise || !noff || !si || !di || !snr_drop || !mixture || !ooff))
        return fail(NHANS_EINVAL, fn + ": null buffer, offsets, indices, SNRs or mixture output with " + std::to_string(njobs) + " jobs to mix");
    std::vector<MixChain> chains;
    std::map<std::tuple<int, int, int64_t>, int> chain_of;      // (0 speech | 1 noise, clip, fitted length) -> chain
    auto chain = [&](int which, int clip, const float* src, int64_t m, int64_t n) {
        auto it = chain_of.find({which, clip, n});
        if (it != chain_of.end()) return it->second;
        chains.push_back({src, (long long)m, (long long)n});
        return chain_of[{which, clip, n}] = (int)chains.size() - 1;
    };
    std::vector<MixJob> jobs((size_t)njobs);
    long long tiles = 0, samples = 0, chained = 0;
    for (int j = 0; j < njobs; ++j) {
        const std::string job = fn + ": job " + std::to_string(j) + ": ";
        const int k = ki ? ki[j] : -1;
        if (si[j] < 0 || si[j] >= nspeech) return fail(NHANS_EINVAL, job + "speech index " + std::to_string(si[j]) + " of " + std::to_string(nspeech) + " clips");
        if (k < -1 || k >= nnoise) return fail(NHANS_EINVAL, job + "keep index " + std::to_string(k) + " of " + std::to_string(nnoise) + " clips");
        if (di[j] < 0 || di[j] >= nnoise) return fail(NHANS_EINVAL, job + "drop index " + std::to_string(di[j]) + " of " + std::to_string(nnoise) + " clips");
        if (k >= 0 && !snr_keep) return fail(NHANS_EINVAL, job + "a keep noise and no keep SNRs");
        const int64_t n = soff[si[j] + 1] - soff[si[j]], ma = k >= 0 ? noff[k + 1] - noff[k] : 1, mb = noff[di[j] + 1] - noff[di[j]];
        if (n < 1) return fail(NHANS_EINVAL, job + "speech clip " + std::to_string(si[j]) + " has " + std::to_string(n) + " samples");
        if (ma < 1) return fail(NHANS_EINVAL, job + "keep noise clip " + std::to_string(k) + " has " + std::to_string(ma) + " samples");
        if (mb < 1) return fail(NHANS_EINVAL, job + "drop noise clip " + std::to_string(di[j]) + " has " + std::to_string(mb) + " samples");
        if (ooff[j + 1] - ooff[j] < n)
            return fail(NHANS_EINVAL, job + "its outputs have room for " + std::to_string(ooff[j + 1] - ooff[j]) + " of " + std::to_string(n) + " samples");
        MixJob& r = jobs[j];
        r = {speech + soff[si[j]], k >= 0 ? noise + noff[k] : nullptr, noise + noff[di[j]], (long long)n, (long long)ma, (long long)mb,
             (long long)ooff[j], tiles, 1.0, 1.0, 0, 0, 0, 0};
        r.ps = chain(0, si[j], r.s, n, n);
        if (k >= 0) r.pa = chain(1, k, r.a, ma, n);
        r.pb = chain(1, di[j], r.b, mb, n);
        if (k >= 0) (void)nhans_mix_snr_factor(snr_keep[j], &r.fa);
        (void)nhans_mix_snr_factor(snr_drop[j], &r.fb);
        tiles += (n + kMixTile - 1) / kMixTile;
        samples += n;
    }
    if (tiles > 0x7fffffffLL) return fail(NHANS_EINVAL, fn + ": too many samples for one call (split it)");
    for (const MixChain& ch : chains) chained += ch.n;
    return ctx_call(c, stream, [&](hipStream_t s) -> int {
        if (njobs == 0) return NHANS_OK;
        WsPlan p;
        MixChain* chains_dev; MixJob* jobs_dev; double* pw; float* peaks;
        p.add(&chains_dev, chains.size());
        p.add(&jobs_dev, jobs.size());
        p.add(&pw, chains.size());
        p.add(&peaks, (size_t)tiles);
        int rc = ws_commit(c, p); if (rc) return rc;
        rc = h2d(c, chains_dev, chains, s); if (rc) return rc;
        rc = h2d(c, jobs_dev, jobs, s); if (rc) return rc;
        const double n = (double)samples, T = (double)tiles, J = (double)njobs;
        const int outs = 1 + (target ? 1 : 0) + (keep ? 1 : 0) + (drop ? 1 : 0);
        {   // per fitted sample: a product and one addition of the chain
            Prof pr(c, s, "mix_power");
            launch_mix_power("mix_power", chains_dev, (int)chains.size(), pw, s);
            pr.done(2.0 * (double)chained, 4.0 * (double)chained + 8.0 * (double)chains.size());
        }
        {   // per sample: two products and two sums
            Prof pr(c, s, "mix_combine");
            launch_mix_combine("mix_combine", jobs_dev, njobs, tiles, pw, mixture, peaks, records, s);
            pr.done(4.0 * n, 16.0 * n + 4.0 * T + (records ? 40.0 * J : 0.0));
        }
        {   // per sample and output: at most a product, a sum and a division
            Prof pr(c, s, "mix_finish");
            launch_mix_finish("mix_finish", jobs_dev, njobs, tiles, pw, peaks, mixture, target, keep, drop, records, s);
            pr.done(3.0 * outs * n, (16.0 + 4.0 * outs) * n + (records ? 24.0 * J : 0.0));
        }
        return NHANS_OK;
    });
}

}  // extern "C"
