// Host check of n-hans_amd/csrc/net_weights.h, which it includes alone (tests/test_net_weights_host.py builds it with the
// address and undefined-behaviour sanitizers and feeds it).  stdin: one "name count" line per array of a blob, a line "--"
// after each blob.  Each array gets a distinct fake pointer; the arrays are resolved as nhans_create_ex resolves a blob's,
// and every pointer the struct then exposes is printed as "field = name of the array it points at" (a null field is not
// printed), after "has_split = 0|1" -- or the one line "refused: <message>"; then "--".  Exit status 0 either way.
#include "../n-hans_amd/csrc/net_weights.h"

#include <cstdio>
#include <iostream>
#include <map>

static void one_blob(const std::vector<std::string>& names, const std::vector<size_t>& counts) {
    std::vector<float> fake(names.size() + 1);
    std::map<std::string, size_t> index;
    for (size_t i = 0; i < names.size(); ++i) index[names[i]] = i;

    NetWeights nw;
    const std::string bad = resolve_net_weights(tower_geometry(200, 201), main_geometry(35, 201),
        [&](const std::string& n, const float** p, size_t* have) {
            const auto it = index.find(n);
            if (it == index.end()) return false;
            *p = &fake[it->second]; *have = counts[it->second];
            return true;
        }, &nw);
    if (!bad.empty()) { std::printf("refused: %s\n", bad.c_str()); return; }

    std::printf("has_split = %d\n", nw.has_split ? 1 : 0);
    auto show = [&](const std::string& field, const float* p) {
        if (!p) return;
        const size_t i = (size_t)(p - fake.data());
        std::printf("%s = %s\n", field.c_str(), i < names.size() ? names[i].c_str() : "?");
    };
    auto show_conv = [&](const std::string& f, const ConvWeights& w) {
        show(f + ".wpk[0]", w.wpk[0]); show(f + ".wpk[1]", w.wpk[1]);
        show(f + ".wpk_t[0]", w.wpk_t[0]); show(f + ".wpk_t[1]", w.wpk_t[1]);
        show(f + ".w", w.w); show(f + ".cb", w.cb); show(f + ".tf", w.tf); show(f + ".tt", w.tt); show(f + ".ff", w.ff);
        show(f + ".idw", w.idw); show(f + ".ws", w.ws); show(f + ".wino_u", w.wino_u); show(f + ".wino_ws", w.wino_ws);
    };
    for (int b = 0; b < 4; ++b) {
        show_conv("tower[" + std::to_string(b) + "].c1", nw.tower[b].c1);
        show_conv("tower[" + std::to_string(b) + "].c2", nw.tower[b].c2);
    }
    for (int b = 0; b < 8; ++b) {
        show_conv("stack[" + std::to_string(b) + "].c1", nw.stack[b].c1);
        show_conv("stack[" + std::to_string(b) + "].c2", nw.stack[b].c2);
    }
    show_conv("head_conv", nw.head_conv);
    show_conv("head_dense", nw.head_dense);
    show("zero", nw.zero); show("tw400", nw.tw400); show("window", nw.window); show("wsyn", nw.wsyn);
    show("cond_w", nw.cond_w); show("cond_base", nw.cond_base); show("ones", nw.ones);
}

int main() {
    std::vector<std::string> names;
    std::vector<size_t> counts;
    std::string name;
    size_t count;
    while (std::cin >> name) {
        if (name != "--") {
            if (!(std::cin >> count)) return 2;
            names.push_back(name); counts.push_back(count);
            continue;
        }
        one_blob(names, counts);
        std::printf("--\n");
        names.clear(); counts.clear();
    }
    return 0;
}
