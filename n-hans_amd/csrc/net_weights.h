// The arrays of the folded blob (fold.py: fold_arrays) that the launch sequences of host_net.hip read, resolved ONCE per
// context.  Every array is declared exactly once in resolve_net_weights() -- its name, its float count and its class --
// and lands in one field of NetWeights; nhans_create_ex() keeps the result, and no launch looks anything up by name.
// Nothing here knows HIP or the context, so the header compiles alone (tests/net_weights_main.cpp).
//   Classes.  required: missing or mis-sized refuses the blob.  split: required when the blob carries split-f16 weights
// (has_split: `head.dense.wpk_h` is present) -- every `*_h` pack and `<conv>.ws` a precision-1 launch dereferences -- and
// not asked for otherwise.  optional pair (`.tt` + `.ff`, `.wino` + `.wino.ws`): both or neither, one without the other
// resolves as neither; present at a wrong size refuses the blob.  A field whose array the block does not have stays null.
#pragma once
#include <cstddef>
#include <string>
#include <vector>

struct BlockGeo {
    int kh, kw, sh, sw, cin, cout, hin, win, hout, wout;
};

inline std::vector<BlockGeo> tower_geometry(int h, int w) {       // SN/main.py:194-198; h x w: one context image
    const int kh[4] = {8, 8, 4, 4}, kw[4] = {4, 4, 4, 4}, sh[4] = {3, 3, 1, 1}, sw[4] = {2, 2, 1, 2};
    const int co[4] = {64, 128, 256, 512};
    std::vector<BlockGeo> v;
    int c = 1;
    for (int i = 0; i < 4; ++i) {
        BlockGeo g{kh[i], kw[i], sh[i], sw[i], c, co[i], h, w, (h + sh[i] - 1) / sh[i], (w + sw[i] - 1) / sw[i]};
        v.push_back(g);
        h = g.hout; w = g.wout; c = g.cout;
    }
    return v;
}

inline std::vector<BlockGeo> main_geometry(int h, int w) {        // SN/main.py:221-229; h x w: one frame window
    const int k[8] = {4, 4, 4, 4, 3, 3, 3, 3}, s[8] = {1, 1, 2, 1, 2, 1, 2, 1};
    const int co[8] = {64, 64, 128, 128, 256, 256, 512, 512};
    std::vector<BlockGeo> v;
    int c = 1;
    for (int i = 0; i < 8; ++i) {
        BlockGeo g{k[i], k[i], s[i], s[i], c, co[i], h, w, (h + s[i] - 1) / s[i], (w + s[i] - 1) / s[i]};
        v.push_back(g);
        h = g.hout; w = g.wout; c = g.cout;
    }
    return v;
}

// One conv.  wpk / wpk_t: [precision] (0: pack_igemm, 1: pack_igemm_h3), wpk_t the 1x1 `_transform` of a
// channel-changing block's conv2; w: the direct one-channel conv; cb: bias row (tower, head); tf / tt / ff: position
// table and its two terms (stack); idw: per-channel weight of the residual; ws: unscale vector of the split packs;
// wino_u / wino_ws: Winograd pack and its unscale vector.
struct ConvWeights {
    const float *wpk[2] = {}, *wpk_t[2] = {};
    const float *w = nullptr, *cb = nullptr, *tf = nullptr, *tt = nullptr, *ff = nullptr, *idw = nullptr, *ws = nullptr;
    const float *wino_u = nullptr, *wino_ws = nullptr;
};
struct BlockWeights {
    ConvWeights c1, c2;
};
struct NetWeights {
    BlockWeights tower[4], stack[8];
    ConvWeights head_conv, head_dense;
    const float *zero = nullptr, *tw400 = nullptr, *window = nullptr, *wsyn = nullptr, *cond_w = nullptr, *cond_base = nullptr;
    const float* ones = nullptr;        // `head.dense.idw`: 256 ones
    bool has_split = false;
};

// find(name, &pointer, &float count) -> is the array in the blob?  -> "" and *nw filled, or the first violation.
template <typename Find>
std::string resolve_net_weights(const std::vector<BlockGeo>& tower, const std::vector<BlockGeo>& stack, Find find, NetWeights* nw) {
    *nw = NetWeights();
    std::string err;
    const float* p;
    size_t have;
    nw->has_split = find("head.dense.wpk_h", &p, &have);
    auto required = [&](const std::string& name, size_t n, const float** slot) {
        if (!err.empty()) return;
        if (find(name, &p, &have) && have == n) *slot = p;
        else err = "folded blob: array '" + name + "' missing or wrong size (want " + std::to_string(n) + ")";
    };
    auto split = [&](const std::string& name, size_t n, const float** slot) { if (nw->has_split) required(name, n, slot); };
    auto optional_pair = [&](const std::string& na, size_t ca, const float** sa, const std::string& nb, size_t cb, const float** sb) {
        if (!err.empty()) return;
        const float *pa = nullptr, *pb = nullptr;
        size_t ha = 0, hb = 0;
        const bool a = find(na, &pa, &ha), b = find(nb, &pb, &hb);
        if (a && ha != ca) err = "folded blob: optional array '" + na + "' has the wrong size (want " + std::to_string(ca) + ")";
        else if (b && hb != cb) err = "folded blob: optional array '" + nb + "' has the wrong size (want " + std::to_string(cb) + ")";
        else if (a && b) { *sa = pa; *sb = pb; }
    };
    // a conv with packed weights: K x N matrix `name`.wpk, its split form and unscale vector
    auto packed = [&](const std::string& conv, size_t K, size_t N, ConvWeights* w) {
        required(conv + ".wpk", K * N, &w->wpk[0]);
        split(conv + ".wpk_h", K * N, &w->wpk[1]);
        split(conv + ".ws", N, &w->ws);
    };
    auto transform = [&](const std::string& conv, size_t K, size_t N, ConvWeights* w) {
        required(conv + ".wpk_t", K * N, &w->wpk_t[0]);
        split(conv + ".wpk_t_h", K * N, &w->wpk_t[1]);
    };

    required("tw400", 800, &nw->tw400);
    required("window", 400, &nw->window);
    required("wsyn", 400, &nw->wsyn);
    required("zero", 16384, &nw->zero);

    for (int b = 0; b < 4; ++b) {
        const BlockGeo& g = tower[b];
        const std::string t = "t" + std::to_string(b);
        BlockWeights& w = nw->tower[b];
        const size_t taps = (size_t)g.kh * g.kw, co = g.cout;
        if (g.cin == 1) required(t + ".c1.w", taps * co, &w.c1.w);
        else packed(t + ".c1", taps * g.cin, co, &w.c1);
        required(t + ".c1.cb", co, &w.c1.cb);
        packed(t + ".c2", taps * co, co, &w.c2);
        if (g.cin == 1) required(t + ".c2.idw", co, &w.c2.idw);
        else transform(t + ".c2", g.cin, co, &w.c2);
        required(t + ".c2.cb", co, &w.c2.cb);
    }

    size_t cond_cols = 0;
    for (int b = 0; b < 8; ++b) {
        const BlockGeo& g = stack[b];
        const std::string m = "m" + std::to_string(b);
        BlockWeights& w = nw->stack[b];
        const size_t taps = (size_t)g.kh * g.kw, co = g.cout;
        if (g.cin == 1) required(m + ".c1.w", taps * co, &w.c1.w);
        else packed(m + ".c1", taps * g.cin, co, &w.c1);
        packed(m + ".c2", taps * co, co, &w.c2);
        if (g.cin != 1 && g.cin != g.cout) transform(m + ".c2", g.cin, co, &w.c2);
        required(m + ".c2.idw", co, &w.c2.idw);
        for (int j = 0; j < 2; ++j) {
            ConvWeights& cw = j ? w.c2 : w.c1;
            const std::string conv = m + (j ? ".c2" : ".c1");
            required(conv + ".tf", (size_t)g.hout * g.wout * co, &cw.tf);
            optional_pair(conv + ".tt", (size_t)g.hout * co, &cw.tt, conv + ".ff", (size_t)g.wout * co, &cw.ff);
            // the 1-D Winograd form (fold.py: wino_eligible, pack_wino): stride-1 4x4 convs of cout -> cout channels
            const bool stride1 = j || (g.sh == 1 && g.sw == 1), square = j || g.cin == g.cout;
            if (g.kh == 4 && g.kw == 4 && stride1 && square)
                optional_pair(conv + ".wino", 8 * (size_t)g.kh * co * co, &cw.wino_u, conv + ".wino.ws", co, &cw.wino_ws);
            cond_cols += co;
        }
    }
    const size_t emb = tower[3].cout;
    required("cond.w", 2 * emb * cond_cols, &nw->cond_w);
    required("cond.base", cond_cols, &nw->cond_base);

    // head: last_conv [stack rows, 1] VALID -> 512, last_dense [columns x 512] -> 201 bins padded to 256
    const BlockGeo& g = stack[7];
    packed("head.conv", (size_t)g.hout * g.cout, 512, &nw->head_conv);
    required("head.conv.cb", 512, &nw->head_conv.cb);
    packed("head.dense", (size_t)g.wout * 512, 256, &nw->head_dense);
    required("head.dense.cb", 256, &nw->head_dense.cb);
    required("head.dense.idw", 256, &nw->ones);
    if (!err.empty()) *nw = NetWeights();
    return err;
}
