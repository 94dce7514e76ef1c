// Stand-alone check of n-hans_amd/csrc/ws_plan.h (tests/test_ws_plan_host.py builds it with the address and undefined
// behaviour sanitizers and runs it): plans placed over a host array.  Exit status 0: every check held.
#include "../n-hans_amd/csrc/ws_plan.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {

int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) { std::printf("%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

struct Run56 { char b[56]; };
static_assert(sizeof(Run56) == 56, "the 56-byte element");

size_t rounded(size_t count, size_t elem) { return (count * elem + 255) & ~(size_t)255; }

template <typename T> T* sentinel() { return reinterpret_cast<T*>(static_cast<uintptr_t>(0x5EED5EED)); }

// counts 0, 1, 63, 64, 65 and `exact`, for which exact * sizeof(T) is a multiple of 256, in that order: every slot is
// base + the running sum, which `off` carries on to the next type
template <typename T> struct Six {
    T* slot[6];
    size_t count[6];
    explicit Six(size_t exact) : count{0, 1, 63, 64, 65, exact} {
        for (T*& s : slot) s = sentinel<T>();
    }
    void declare(WsPlan& p) { for (int i = 0; i < 6; ++i) p.add(&slot[i], count[i]); }
    void expect(const char* base, size_t* off) const {
        for (int i = 0; i < 6; ++i) {
            CHECK(reinterpret_cast<const char*>(slot[i]) == base + *off);
            *off += rounded(count[i], sizeof(T));
        }
    }
    bool untouched() const {
        for (T* s : slot) if (s != sentinel<T>()) return false;
        return true;
    }
};

void layout() {
    Six<char> a(512);
    Six<float> b(128);
    Six<double> c(32);
    Six<Run56> d(32);
    CHECK((32 * sizeof(Run56)) % 256 == 0);
    WsPlan p;
    a.declare(p); b.declare(p); c.declare(p); d.declare(p);
    CHECK(p.ok());
    CHECK(a.untouched() && b.untouched() && c.untouched() && d.untouched());      // add() writes no pointer
    std::vector<char> arena(p.bytes() + 256, (char)0xA5);
    CHECK(p.place(arena.data()));
    size_t off = 0;
    a.expect(arena.data(), &off); b.expect(arena.data(), &off); c.expect(arena.data(), &off); d.expect(arena.data(), &off);
    CHECK(p.bytes() == off);
    CHECK(off % 256 == 0 && off > 0);
    // a count of 0 is the address of what comes next
    CHECK(reinterpret_cast<char*>(a.slot[0]) == reinterpret_cast<char*>(a.slot[1]));
    CHECK(reinterpret_cast<char*>(d.slot[0]) == reinterpret_cast<char*>(d.slot[1]));
    for (char ch : arena) if (ch != (char)0xA5) { CHECK(!"place() wrote into the array"); break; }
}

void zero_count() {
    WsPlan p;
    float *x = nullptr, *z = nullptr, *y = nullptr, *last = nullptr;
    p.add(&x, 3);
    const size_t before = p.bytes();
    p.add(&z, 0);
    CHECK(p.bytes() == before);
    p.add(&y, 5);
    p.add(&last, 0);                        // (nothing follows: the end of the plan)
    char arena[512];
    CHECK(p.place(arena));
    CHECK(reinterpret_cast<char*>(x) == arena && reinterpret_cast<char*>(z) == arena + 256 && z == y);
    CHECK(reinterpret_cast<char*>(last) == arena + 512 && p.bytes() == 512);
    WsPlan empty;
    CHECK(empty.bytes() == 0 && empty.place(nullptr));
}

// head, then two branches that share their place; `first` / `second` floats in the branches' single buffers
void overlap(size_t first, size_t second) {
    WsPlan p;
    double* head = nullptr; float *a = nullptr, *a2 = nullptr, *b = nullptr; char* tail = nullptr;
    p.add(&head, 10);
    const size_t m = p.mark();
    CHECK(m == 256);
    p.add(&a, first);
    p.add(&a2, 1);
    p.rewind(m);
    p.add(&b, second);
    const size_t want = 256 + (rounded(first, 4) + 256 > rounded(second, 4) ? rounded(first, 4) + 256 : rounded(second, 4));
    CHECK(p.bytes() == want);
    p.add(&tail, 1);                        // (follows the SECOND branch, wherever the peak is)
    std::vector<char> arena(p.bytes());
    CHECK(p.place(arena.data()));
    CHECK(reinterpret_cast<char*>(a) == arena.data() + m && reinterpret_cast<char*>(b) == arena.data() + m);
    CHECK(reinterpret_cast<char*>(a2) == arena.data() + m + rounded(first, 4));
    CHECK(tail == arena.data() + m + rounded(second, 4));
}

void nested_overlap() {
    WsPlan p;
    char *h = nullptr, *o1 = nullptr, *i1 = nullptr, *i2 = nullptr, *o2 = nullptr, *o3 = nullptr;
    p.add(&h, 100);                         // [0, 256)
    const size_t outer = p.mark();
    p.add(&o1, 300);                        // [256, 768)
    const size_t inner = p.mark();
    p.add(&i1, 2000);                       // [768, 2816): the peak
    p.rewind(inner);
    p.add(&i2, 10);                         // [768, 1024)
    p.add(&o2, 10);                         // [1024, 1280)
    p.rewind(outer);
    p.add(&o3, 600);                        // [256, 1024)
    CHECK(outer == 256 && inner == 768 && p.bytes() == 2816);
    std::vector<char> arena(p.bytes());
    char* base = arena.data();
    CHECK(p.place(base));
    CHECK(h == base && o1 == base + 256 && i1 == base + 768 && i2 == base + 768 && o2 == base + 1024 && o3 == base + 256);
}

void never_placed() {
    Six<float> s(64);
    {
        WsPlan p;
        s.declare(p);
        CHECK(p.bytes() > 0);
    }
    CHECK(s.untouched());
}

void overflow() {
    std::vector<float*> slot(WsPlan::kCap + 5, sentinel<float>());
    WsPlan p;
    for (int i = 0; i < WsPlan::kCap; ++i) p.add(&slot[i], 1);
    CHECK(p.ok() && p.bytes() == (size_t)WsPlan::kCap * 256);
    for (int i = WsPlan::kCap; i < WsPlan::kCap + 5; ++i) p.add(&slot[i], 1);
    CHECK(!p.ok());
    std::vector<char> arena((size_t)(WsPlan::kCap + 5) * 256);
    CHECK(!p.place(arena.data()));          // the refusal, and no pointer of a plan that is not whole
    for (float* s : slot) CHECK(s == sentinel<float>());
}

}  // namespace

int main() {
    layout();
    zero_count();
    overlap(1000, 10);
    overlap(10, 1000);
    overlap(64, 128);
    nested_overlap();
    never_placed();
    overflow();
    if (failures) std::printf("%d check(s) failed\n", failures);
    return failures ? 1 : 0;
}
