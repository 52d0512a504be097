// Stand-alone host check of rt_gather_layout.hpp (what the one-bounce diffuse gather adds to the layout arithmetic of rt_ao_layout.hpp, and
// the argument rule of its calls), meant for a sanitizer build on the CPU:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iraytracer-in-cpp_amd/csrc tools/gather_layout_check.cpp -o gather_layout_check
// (make -C raytracer-in-cpp_amd/csrc gather_check builds and runs it).  Exit status 0: every check held.
#include <cstdio>
#include <vector>

#include "rt_gather_layout.hpp"

using namespace rtamd;

static int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

// The owner's sum as the kernel takes it: a staging array of 64 entries per round that lane l fills with what it holds, then lane p reads
// [first, first + count).  Every read must stay inside the array, be a lane that holds a ray of point p (ao_slot), and over the rounds the
// reads of lane p must be the directions 0, 1, .. K - 1 of point p in this order; a lane that owns no point reads nothing.
static void owners(const int32_t m) {
    const AoLayout L = ao_layout(m);
    CHECK(L.group * L.K == L.rounds * 64);
    for (int32_t p = 0; p < 64; ++p) {
        int32_t next = 0;
        for (int32_t round = 0; round < L.rounds; ++round) {
            std::vector<int32_t> staged_p(64), staged_k(64);          // (a vector, so that the sanitizer sees a read outside it)
            for (int32_t lane = 0; lane < 64; ++lane) {
                const AoSlot s = ao_slot(1 << 20, L, 0, round, lane);
                staged_p[lane] = s.p; staged_k[lane] = s.k;
            }
            const GatherRange r = gather_range(L, p, round);
            CHECK(r.count >= 0 && r.first >= 0 && r.first + r.count <= 64);
            unsigned long long bits = 0ull;
            for (int32_t q = r.first; q < r.first + r.count; ++q) {
                CHECK(staged_p.at(q) == p && staged_k.at(q) == next && staged_k.at(q) == r.k0 + (q - r.first));
                ++next;
                bits |= 1ull << q;
            }
            CHECK(bits == ao_point_lanes(L, p, round));
        }
        CHECK(next == (p < L.group ? L.K : 0));
    }
}

int main() {
    for (int32_t m = 1; m <= kAoMaxGrid; ++m) owners(m);
    // the argument rule
    float a[64], b[64], o[64];
    CHECK(gather_args(4, a, b, 3, o) == nullptr);
    CHECK(gather_args(0, nullptr, nullptr, 3, nullptr) == nullptr);
    CHECK(gather_args(-1, a, b, 3, o) != nullptr);
    CHECK(gather_args(4, a, b, 0, o) != nullptr && gather_args(4, a, b, 17, o) != nullptr && gather_args(0, nullptr, nullptr, 0, nullptr) != nullptr);
    CHECK(gather_args(4, a, b, 1, o) == nullptr && gather_args(4, a, b, 16, o) == nullptr);
    CHECK(gather_args(4, nullptr, b, 3, o) != nullptr && gather_args(4, a, nullptr, 3, o) != nullptr && gather_args(4, a, b, 3, nullptr) != nullptr);
    CHECK(gather_args(4, a, b, 3, a) != nullptr && gather_args(4, a, b, 3, b) != nullptr);
    CHECK(gather_args(4, a, b, 3, a + 11) != nullptr);                       // the last float of the input
    CHECK(gather_args(4, a, b, 3, a + 12) == nullptr);                       // directly behind it
    CHECK(gather_args(4, a + 12, b, 3, a) == nullptr && gather_args(4, a + 11, b, 3, a) != nullptr);
    CHECK(gather_args(0x7fffffff, a, b, 3, o) != nullptr);                   // (n * 12 bytes in size_t: 24 GB ranges of neighbours on the stack overlap)
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("rt_gather_layout.hpp: all checks held\n");
    return 0;
}
