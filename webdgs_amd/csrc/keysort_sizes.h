// The sizing of the stable u64 key sort (keysort.hip): how S slots are tiled over workgroups, the words of a pass's digit table, and what a KeySort reserves
// for sorts of two sizes.  Plain C++17 like alloc_cache.h and devmem.h, with no HIP in it: tests/cpp/keysort_sizes_test.cpp checks it on the CPU.
#pragma once
#include <algorithm>
#include <cstdint>

namespace wdgs {

constexpr uint32_t KS_THREADS = 256;
constexpr uint32_t KS_RADIX_BITS = 8;
constexpr uint32_t KS_RADIX = 1u << KS_RADIX_BITS;
constexpr uint32_t KS_CHUNKS = 16;                        // chunks of 64 pairs a wave holds in registers
constexpr uint32_t KS_SUBTILE = KS_THREADS * KS_CHUNKS;   // 4096: what a workgroup ranks between two barriers
constexpr uint32_t KS_MAX_WORKGROUPS = 8192;              // the digit table has KS_RADIX * workgroups <= 2 097 152 words: within what the scan is tested to

// The tiling of S slots: workgroup g owns [g * tile, min(S, (g + 1) * tile)), tile a multiple of KS_SUBTILE
struct KeySortTiling { uint32_t S, tile, workgroups; };

// (64-bit sums: S + 8191 does not fit 32 bits for the last 8191 sizes below 2^32)
inline KeySortTiling keysort_tiling(uint32_t S) {
    const uint64_t per = ((uint64_t)S + KS_MAX_WORKGROUPS - 1u) / KS_MAX_WORKGROUPS;
    const uint64_t tile = std::max<uint64_t>(KS_SUBTILE, (per + KS_SUBTILE - 1u) / KS_SUBTILE * KS_SUBTILE);
    return KeySortTiling{S, (uint32_t)tile, (uint32_t)(((uint64_t)S + tile - 1u) / tile)};
}

// The words of the digit-major table (and of its scan) for S slots
inline uint32_t keysort_table_words(uint32_t S) { return S == 0u ? 0u : KS_RADIX * keysort_tiling(S).workgroups; }

// What sorts of S_a and of S_b slots need together: n pairs, flags and ids; table_words of table and of offsets, and 2 * table_words / KS_RADIX words of
// or_and; a scan of scan_words elements.  The tile doubles past 8192 * 4096 slots, so the larger S can have the smaller table: the table is the larger of the two.
struct KeySortSizes { uint32_t n, table_words, scan_words; };
inline KeySortSizes keysort_reserve_sizes(uint32_t S_a, uint32_t S_b) {
    const uint32_t n = std::max(S_a, S_b), table_words = std::max(keysort_table_words(S_a), keysort_table_words(S_b));
    return KeySortSizes{n, table_words, std::max(n, table_words)};
}

}  // namespace wdgs
