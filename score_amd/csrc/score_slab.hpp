// score_slab.hpp -- one allocation cut into typed regions.  Each region is declared once with its element type and count; it
// gives its typed pointer in any copy of the slab -- device memory, a pinned or host-mapped block, a staging vector -- so the
// device view and the host view of a piece come from the same declaration.  A slab rounds every region up to `align` bytes and
// gives it `least` bytes at least: 256 and 8 by default (pieces a kernel may fill or upload on their own); (8, 0) packs
// doubles back to back, (4, 0) 32-bit words.
#pragma once

#include <algorithm>
#include <cstddef>
#include <utility>

template <class T> struct Region { size_t off = 0; T* in(void* base) const { return (T*)((char*)base + off); } };
struct Slab {
    size_t bytes = 0, align, least;
    Slab(size_t align_ = 256, size_t least_ = 8) : align(align_), least(least_) {}
    template <class T> Region<T> add(size_t count) {
        return Region<T>{std::exchange(bytes, bytes + ((std::max<size_t>(count * sizeof(T), least) + align - 1) & ~(align - 1)))};
    }
};
