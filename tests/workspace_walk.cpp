// workspace_walk.cpp -- a stand-alone host program over csrc/workspace.h alone (tests/test_workspace_walk_cpu.py compiles and runs it):
// for a handful of region lists with mixed element sizes and alignments, zero-count regions included, a measuring walk (null base) and a
// real walk over a malloc'ed buffer must take the same offsets and the same total; every pointer of the measuring walk is null, every real
// pointer is aligned as asked, no two regions overlap and the last one ends at or before the total. Exit status 0 and "ok", or the first
// violated statement on stderr and status 1.
#include "workspace.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

struct Region { int elem; size_t count, align; };       // elem: sizeof the element type, one of 1, 2, 4, 8, 16

struct Taken { size_t before, after; char* p; };

struct alignas(16) Quad { unsigned v[4]; };

static Taken take(ls::WsWalk& w, const Region& r) {
    Taken t;
    t.before = w.bytes();
    switch (r.elem) {
    case 1: t.p = (char*)w.take<unsigned char>(r.count, r.align); break;
    case 2: t.p = (char*)w.take<unsigned short>(r.count, r.align); break;
    case 4: t.p = (char*)w.take<int>(r.count, r.align); break;
    case 8: t.p = (char*)w.take<double>(r.count, r.align); break;
    default: t.p = (char*)w.take<Quad>(r.count, r.align); break;
    }
    t.after = w.bytes();
    return t;
}

#define CHECK(cond, ...)                                             \
    do {                                                             \
        if (!(cond)) {                                               \
            std::fprintf(stderr, "list %d region %d: ", li, (int)i); \
            std::fprintf(stderr, __VA_ARGS__);                       \
            std::fprintf(stderr, "\n");                              \
            return 1;                                                \
        }                                                            \
    } while (0)

int main() {
    const std::vector<std::vector<Region>> lists = {
        // the shape of most families: 256-byte regions of mixed types, a zero-count one in the middle
        {{1, 1000, 256}, {4, 1000, 256}, {4, 1001, 256}, {8, 0, 256}, {4, 1, 256}, {8, 37, 256}},
        // packed at 4 bytes (the sort users of assemble.hip)
        {{4, 7, 4}, {4, 7, 4}, {4, 8, 4}, {1, 4 * 531, 4}},
        // natural alignment (normals.hip, meshgeom.hip): doubles, then floats
        {{8, 3 * 1024, 8}, {4, 4, 4}, {4, 3 * 5, 4}, {4, 9 * 7, 4}},
        // alignments that go up and down: an odd byte count before doubles, a 16-byte type, a 64-byte region behind a 256-byte one
        {{1, 3, 1}, {8, 2, 8}, {2, 5, 2}, {16, 3, 16}, {4, 129, 256}, {4, 16, 64}, {4, 9, 4}, {1, 0, 1}, {8, 1, 8}},
        // nothing but empty regions, and no region at all
        {{4, 0, 256}, {8, 0, 8}, {1, 0, 1}},
        {},
        // one byte
        {{1, 1, 256}},
    };
    for (int li = 0; li < (int)lists.size(); ++li) {
        const std::vector<Region>& L = lists[li];
        ls::WsWalk measure(nullptr);
        std::vector<Taken> m;
        for (const Region& r : L) m.push_back(take(measure, r));
        const size_t total = measure.bytes();
        // a base as the device allocator gives it: 256-byte aligned (ws_align_base is what the sort users do to a caller's pointer)
        void* raw = std::malloc(total + 256 + 1);
        if (!raw) return 2;
        std::memset(raw, 0xab, total + 256 + 1);
        char* base = ls::ws_align_base(raw, 256);
        size_t i = 0;
        CHECK(((uintptr_t)base & 255) == 0 && base >= (char*)raw && base < (char*)raw + 256, "ws_align_base gave %p for %p", (void*)base, raw);
        ls::WsWalk real(base);
        size_t end = 0;
        for (i = 0; i < L.size(); ++i) {
            const Taken t = take(real, L[i]);
            const size_t bytes = L[i].count * (size_t)L[i].elem;
            CHECK(m[i].p == nullptr, "the measuring walk formed a pointer");
            CHECK(t.before == m[i].before && t.after == m[i].after, "offsets differ: measured %zu..%zu, real %zu..%zu", m[i].before, m[i].after,
                  t.before, t.after);
            CHECK(t.p != nullptr, "the real walk returned null");
            const size_t off = (size_t)(t.p - base);
            CHECK(((uintptr_t)t.p & (L[i].align - 1)) == 0, "pointer at offset %zu is not aligned to %zu", off, L[i].align);
            CHECK(off >= end, "region at %zu overlaps the one before, which ends at %zu", off, end);
            CHECK(off >= t.before && off + bytes <= t.after, "region %zu..%zu is outside what the walk advanced over (%zu..%zu)", off, off + bytes,
                  t.before, t.after);
            std::memset(t.p, (int)i, bytes);            // (a sanitizer build sees every byte of every region written)
            end = off + bytes;
        }
        CHECK(real.bytes() == total, "totals differ: measured %zu, real %zu", total, real.bytes());
        CHECK(end <= total, "the last region ends at %zu, past the total %zu", end, total);
        CHECK((unsigned char)base[total] == 0xab, "the byte behind the total was written");
        std::free(raw);
    }
    std::puts("ok");
    return 0;
}
