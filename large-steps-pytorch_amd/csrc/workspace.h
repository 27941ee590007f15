// workspace.h -- the one walk over the regions of a device buffer: the same sequence of take() calls measures a workspace (null base) and
// carves it (the caller's base), so a region cannot be in a layout without being in its size. Host-only, plain C++, no HIP types.
//
// A family states its workspace as ONE function of (base, sizes) that returns typed pointers and the total; its *_bytes entry point calls it
// with a null base, its launching entry points with the real one. The offsets that function yields are part of the family's contract: its
// kernels were written (and measured) for the alignment of every region relative to the base, so a layout is never "tidied" -- a family
// that packs at 4 bytes behind a rounded-up base keeps doing so through `align`.
#pragma once
#include <cstddef>
#include <cstdint>

namespace ls {

static inline size_t ws_round(size_t x, size_t align) { return (x + align - 1) & ~(align - 1); }          // align: a power of two

// a caller's base rounded up to `align` (the sort users of assemble.hip, which pay `align` bytes of their total for it)
static inline char* ws_align_base(void* p, size_t align = 256) { return (char*)ws_round((uintptr_t)p, align); }

struct WsWalk {
    char* base;              // nullptr: measure only (no pointer is ever formed from it)
    size_t off = 0;
    explicit WsWalk(const void* b) : base((char*)b) {}
    // `count` elements of T at the next multiple of `align`, the region's bytes rounded up to `align`; nullptr when measuring
    template <class T>
    T* take(size_t count, size_t align = 256) {
        off = ws_round(off, align);
        T* p = base ? (T*)(base + off) : nullptr;
        off += ws_round(count * sizeof(T), align);
        return p;
    }
    size_t bytes() const { return off; }
};

}  // namespace ls
