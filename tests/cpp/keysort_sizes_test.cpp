// CPU test of webdgs_amd/csrc/keysort_sizes.h: the tiling of the stable u64 key sort at the sizes where it takes another path (nothing, one subtile and its
// edges, the last size with tiles of 4096 and the first with larger ones, the largest sizes its two users accept), the table's fall where the tile
// doubles, and what a KeySort reserves for a pair of sizes.  Built and run by tests/test_keysort_sizes.py (g++; no GPU, no HIP).
#include <cstdint>
#include <cstdio>

#include "../../webdgs_amd/csrc/keysort_sizes.h"

#define CHECK(cond)                                                                                                   \
    do {                                                                                                              \
        if (!(cond)) { std::printf("FAILED line %d (S = %llu): %s\n", __LINE__, (unsigned long long)S, #cond); return 1; } \
    } while (0)

int main() {
    using namespace wdgs;
    const uint32_t EDGE = 8192u * 4096u;   // the last S whose tile is one subtile
    const uint32_t sizes[] = {0u, 1u, 3u, 4095u, 4096u, 4097u, EDGE, EDGE + 1u, 0x7FFFFFFFu, 0xFFFFFFFDu};
    for (const uint32_t S : sizes) {
        const KeySortTiling t = keysort_tiling(S);
        const uint32_t words = keysort_table_words(S);
        CHECK(t.S == S);
        CHECK(t.tile != 0u && t.tile % 4096u == 0u);
        CHECK(t.workgroups <= 8192u);
        if (S == 0u) {
            CHECK(t.workgroups == 0u && words == 0u);
            continue;
        }
        CHECK((uint64_t)t.workgroups * t.tile >= S);
        CHECK((uint64_t)(t.workgroups - 1u) * t.tile < S);
        CHECK(words == 256u * t.workgroups);
        CHECK(words <= 2097152u);
    }
    uint32_t S = EDGE;
    CHECK(keysort_tiling(S).tile == 4096u && keysort_table_words(S) == 2097152u);
    S = EDGE + 1u;
    CHECK(keysort_tiling(S).tile == 8192u && keysort_table_words(S) == 256u * 4097u);
    CHECK(keysort_table_words(EDGE + 1u) < keysort_table_words(EDGE));   // not monotone
    for (int swap = 0; swap < 2; swap++) {   // the larger table comes from the smaller S, whichever argument carries it
        const KeySortSizes r = swap ? keysort_reserve_sizes(EDGE, EDGE + 1u) : keysort_reserve_sizes(EDGE + 1u, EDGE);
        CHECK(r.n == EDGE + 1u && r.table_words == keysort_table_words(EDGE) && r.scan_words == EDGE + 1u);
    }
    S = 3u;   // a small sort's scan is sized by its table
    const KeySortSizes one = keysort_reserve_sizes(3u, 0u);
    CHECK(one.n == 3u && one.table_words == 256u && one.scan_words == 256u);
    const KeySortSizes two = keysort_reserve_sizes(20481u, 40000u);
    CHECK(two.n == 40000u && two.table_words == 256u * 10u && two.scan_words == 40000u);
    const KeySortSizes none = keysort_reserve_sizes(0u, 0u);
    CHECK(none.n == 0u && none.table_words == 0u && none.scan_words == 0u);
    std::printf("keysort_sizes: ok\n");
    return 0;
}
