// lba_arena.hpp — the arena of a tracker call, on the host: typed sections at 256-byte offsets (ArenaLayout), a host
// image of the leading ones (ArenaImage), and the plan of a call whose sections come as inputs (one upload), outputs
// (one download) and device-only work (ArenaPlan).  Host-only and free of HIP: tests/native/arena_harness.cpp builds
// it with g++.
#pragma once

#include <cassert>
#include <cstddef>
#include <cstring>
#include <vector>

// `count` elements of T at byte `off` of an arena
template <typename T>
struct Sec {
    size_t off = 0, count = 0;
    // The one place where an arena offset becomes a typed pointer: `base` is the arena (the device allocation or a
    // host image) from byte `origin` on.
    T* at(char* base, size_t origin = 0) const { return reinterpret_cast<T*>(base + (off - origin)); }
    const T* at(const char* base, size_t origin = 0) const { return reinterpret_cast<const T*>(base + (off - origin)); }
};

struct ArenaLayout {
    size_t total = 0;
    template <typename T>
    Sec<T> take(size_t count) {
        const Sec<T> s{total, count};
        total += (count * sizeof(T) + 255) & ~size_t(255);
        return s;
    }
};

// host image of an arena's leading sections (the upload); `lay` goes on handing out the sections behind it
struct ArenaImage {
    ArenaLayout lay;
    std::vector<char> bytes;
    template <typename T>
    Sec<T> put(const T* p, size_t count) {
        const Sec<T> s = lay.take<T>(count);
        bytes.resize(lay.total, 0);
        if (count) std::memcpy(bytes.data() + s.off, p, count * sizeof(T));
        return s;
    }
    template <typename T>
    Sec<T> put(const std::vector<T>& v) { return put(v.data(), v.size()); }
};

// The sections of a call in the order the copies need: inputs [0, up_end), outputs [up_end, down_end), work behind
// them.  The plan keeps the two ranges; a pinned host image covers [0, down_end).  A work section may still be added
// once the image is filled (its size may depend on it).  An input behind an output, or either behind a work section,
// would move a range under a copy: a programming error, asserted and kept in `misordered`.
struct ArenaPlan {
    ArenaLayout lay;
    size_t up_end = 0, down_end = 0;
    bool misordered = false;
    template <typename T>
    Sec<T> in(size_t count) { return add<T>(0, count); }
    template <typename T>
    Sec<T> out(size_t count) { return add<T>(1, count); }
    template <typename T>
    Sec<T> work(size_t count) { return add<T>(2, count); }
    size_t total() const { return lay.total; }
    bool over_2gb() const { return lay.total > (size_t(1) << 31); }   // the size limit of the calls that have one

private:
    int stage = 0;   // 0 inputs, 1 outputs, 2 work: never goes back
    template <typename T>
    Sec<T> add(int kind, size_t count) {
        assert(kind >= stage && "ArenaPlan: in, out, work in this order");
        if (kind < stage) misordered = true;
        else stage = kind;
        const Sec<T> s = lay.take<T>(count);
        if (kind == 0) up_end = lay.total;
        if (kind <= 1) down_end = lay.total;
        return s;
    }
};
