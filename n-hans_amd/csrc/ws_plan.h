// The layout of one call's device scratch.  A buffer is declared ONCE -- add(&ptr, count) -- and both its size and its
// place follow from that declaration: place(base) gives every declared pointer base + its offset, bytes() is what the
// whole plan needs.  Nothing here knows HIP or the context (host_ctx.hip: ws_commit reserves bytes() of the context's
// workspace and places the plan there), so the header compiles alone (tests/ws_plan_main.cpp).
//   Each buffer takes count * sizeof(T) bytes rounded up to 256; offsets accumulate in declaration order.  A count of 0
// takes nothing: its pointer is the address of whatever is declared next.
//   Pointers are written by place() only -- after the reserve, which may free and reallocate the workspace.
//   Overlap: m = mark(); ...; rewind(m); buffers added after the rewind start where the mark was taken, and bytes() is
// the peak, not the last top.
//   The entries are a fixed inline array (no allocation per call).  An add() past kCap records nothing but the refusal:
// ok() is false from then on and place() does nothing and returns false.
#pragma once
#include <cstddef>

struct WsPlan {
    static constexpr int kCap = 40;     // the largest plan, nhans_enhance_clips with its phase refinement, declares 35 (a live push: 27)
    static constexpr size_t round_up(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

    template <typename T> void add(T** slot, size_t count) {
        if (n_ == kCap) { overflow_ = true; return; }
        e_[n_++] = {slot, [](void* p, char* at) { *static_cast<T**>(p) = reinterpret_cast<T*>(at); }, top_};
        top_ += round_up(count * sizeof(T));
        if (top_ > peak_) peak_ = top_;
    }
    size_t mark() const { return top_; }
    void rewind(size_t m) { top_ = m; }
    size_t bytes() const { return peak_; }
    bool ok() const { return !overflow_; }
    bool place(char* base) const {
        if (overflow_) return false;
        for (int i = 0; i < n_; ++i) e_[i].set(e_[i].slot, base + e_[i].off);
        return true;
    }

private:
    struct Entry {
        void* slot;
        void (*set)(void* slot, char* at);
        size_t off;
    };
    Entry e_[kCap];
    int n_ = 0;
    bool overflow_ = false;
    size_t top_ = 0, peak_ = 0;
};
