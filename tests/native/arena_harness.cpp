// Host build of the tracker's call arena (amc-slam_amd/csrc/lba_arena.hpp alone, no HIP) for tests/test_arena_host.py:
// a plan is played from a list of (kind, element size, count) and its offsets, ranges and flags are handed back; the
// typed accessor and the host image are probed on small buffers.
// NDEBUG: the plan's assert on a forbidden order would end the process; the test reads the sticky flag instead.
#define NDEBUG
#include <type_traits>

#include "../../amc-slam_amd/csrc/lba_arena.hpp"

namespace {

template <int N>
struct Blob {
    char b[N];
};

template <typename T>
size_t add(ArenaPlan& p, int kind, size_t count) {
    return (kind == 0 ? p.in<T>(count) : kind == 1 ? p.out<T>(count) : p.work<T>(count)).off;
}

// the element sizes of the four entry points' sections (the ABI's structs and the device records)
#define ARENA_SIZES X(4) X(8) X(16) X(20) X(24) X(40) X(64) X(80) X(88) X(96) X(112) X(120) X(168)

static_assert(std::is_same<decltype(Sec<int>{}.at((char*)nullptr)), int*>::value, "a char* base gives T*");
static_assert(std::is_same<decltype(Sec<int>{}.at((const char*)nullptr)), const int*>::value, "a const base gives const T*");

}  // namespace

extern "C" {

// kind[i]: 0 in, 1 out, 2 work.  off[n]; ends = {up_end, down_end, total}.  Returns misordered | over_2gb << 1, or -1
// for an element size the list above does not have.
int arena_plan(int n, const int* kind, const int* elem, const unsigned long long* count, unsigned long long* off,
               unsigned long long* ends) {
    ArenaPlan p;
    for (int i = 0; i < n; ++i) {
        switch (elem[i]) {
#define X(N) case N: off[i] = add<Blob<N>>(p, kind[i], (size_t)count[i]); break;
            ARENA_SIZES
#undef X
            default: return -1;
        }
    }
    ends[0] = p.up_end; ends[1] = p.down_end; ends[2] = p.total();
    return (p.misordered ? 1 : 0) | (p.over_2gb() ? 2 : 0);
}

// Sec<double>{off, 3}.at(base, origin) as a byte distance from base
long long arena_at(unsigned long long off, unsigned long long origin) {
    static char buf[4096];
    const Sec<double> s{(size_t)off, 3};
    const char* cb = buf;
    if (reinterpret_cast<const char*>(s.at(cb, (size_t)origin)) != reinterpret_cast<char*>(s.at(buf, (size_t)origin))) return -1;
    return reinterpret_cast<char*>(s.at(buf, (size_t)origin)) - buf;
}

// an image of two int arrays and a layout section behind them: offs = {a, b, behind, image bytes, layout total};
// returns 1 when the image holds both arrays at their offsets (read back through the typed accessor)
int arena_image(const int* a, int na, const int* b, int nb, int n_behind, unsigned long long* offs) {
    ArenaImage im;
    const Sec<int> sa = im.put(a, (size_t)na);
    const Sec<int> sb = im.put(std::vector<int>(b, b + nb));
    const size_t bytes = im.bytes.size();
    const Sec<double> sc = im.lay.take<double>((size_t)n_behind);
    offs[0] = sa.off; offs[1] = sb.off; offs[2] = sc.off; offs[3] = bytes; offs[4] = im.lay.total;
    const char* base = im.bytes.data();
    return sa.count == (size_t)na && sb.count == (size_t)nb && (!na || !std::memcmp(sa.at(base), a, na * sizeof(int))) &&
           (!nb || !std::memcmp(sb.at(base), b, nb * sizeof(int)));
}

}
