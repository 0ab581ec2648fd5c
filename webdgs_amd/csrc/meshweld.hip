// Welding a triangle soup on the device: a stable u64 key sort, head flags, a scan and a gather (no counterpart in the reference, which
// renders colour only).
//
// S = 3F slots carry keys u64[S]; the distinct keys in ascending order are the vertices, every slot's face index is the rank of its key, and a vertex takes
// the position and colour bits of the LOWEST slot that carries its key.  The sort is an LSD radix sort of (key, slot) pairs by 8-bit digits.  Every pass is
// stable and the slots start ascending, so after the last pass equal keys lie together in ascending slot order and the head of a run is its lowest slot.
// Everything is integer work and every output is a function of the input alone.
//
// No kernel here reads what another workgroup of the same launch writes, and there is no global atomic at all: every kernel reads what earlier launches wrote,
// with plain loads.  A pass is three launches -- histogram, the library's scan over the digit-major table, scatter -- and the order between workgroups comes
// from the scanned table alone: no workgroup waits for another, polls a flag or looks back at a neighbour's partial result.
//
// Which passes run is decided on the device: mw_key_bits leaves every tile's OR and AND of its keys, mw_plan folds them, marks the passes whose digit differs
// somewhere (a bit set in OR ^ AND) and deals them the buffers in turn
// (0 = the caller's keys with slot = index, 1 and 2 = the welder's pairs).  The kernels of a pass whose digit is the same in every key return at once, so
// the host waits a single time, for V, and reads the plan's pass count with it.
#include <algorithm>
#include <memory>

#include "launch.h"

namespace {

typedef unsigned long long u64;

constexpr u32 MW_THREADS = 256;
constexpr u32 MW_WAVES = MW_THREADS / 64;
constexpr u32 MW_RADIX_BITS = 8;
constexpr u32 MW_RADIX = 1u << MW_RADIX_BITS;
constexpr u32 MW_PASSES = 64 / MW_RADIX_BITS;
constexpr u32 MW_CHUNKS = 16;                              // chunks of 64 pairs a wave holds in registers
constexpr u32 MW_SUBTILE = MW_THREADS * MW_CHUNKS;         // 4096: what a workgroup ranks between two barriers
constexpr u32 MW_MAX_WORKGROUPS = 8192;                    // the digit table has MW_RADIX * workgroups <= 2 097 152 words: within what the scan is tested to
static_assert(MW_THREADS == MW_RADIX, "one thread per digit in the scatter's table phases");

// The counters block, u32 words: V, the passes run, the buffer that holds the sorted pairs, a spare, then per pass: run, input buffer, output buffer
constexpr u32 MW_C_TOTAL = 0, MW_C_PASSES = 1, MW_C_FINAL = 2, MW_C_RUN = 4, MW_C_IN = 12, MW_C_OUT = 20, MW_C_WORDS = 28;

struct WeldBuffers {
    const u64* keys0;   // buffer 0: the caller's keys; slot = index
    u64* keys[2];       // buffers 1 and 2
    u32* slots[2];
    __device__ __forceinline__ const u64* keys_of(u32 b) const { return b == 0u ? keys0 : keys[b - 1u]; }
    __device__ __forceinline__ const u32* slots_of(u32 b) const { return b == 0u ? nullptr : slots[b - 1u]; }
};

// The tiling of S slots: workgroup g owns [g * tile, min(S, (g + 1) * tile)), tile a multiple of MW_SUBTILE
struct WeldTiling { u32 S, tile, workgroups; };

__device__ __forceinline__ u32 digit_of(u64 key, u32 pass) { return (u32)(key >> (pass * MW_RADIX_BITS)) & (MW_RADIX - 1u); }

// The OR and the AND of the workgroup's values, in every thread: shuffles inside a wave, then the four waves' words through LDS
__device__ __forceinline__ void block_or_and(u64& o, u64& a, u64 (*lds)[2]) {
#pragma unroll
    for (u32 d = 32; d >= 1; d >>= 1) {
        o |= __shfl_xor(o, (int)d, 64);
        a &= __shfl_xor(a, (int)d, 64);
    }
    if ((threadIdx.x & 63u) == 0u) {
        lds[threadIdx.x >> 6][0] = o;
        lds[threadIdx.x >> 6][1] = a;
    }
    __syncthreads();
    o = 0ull;
    a = ~0ull;
#pragma unroll
    for (u32 w = 0; w < MW_WAVES; w++) {
        o |= lds[w][0];
        a &= lds[w][1];
    }
}

// or_and[2 g], or_and[2 g + 1]: the OR and the AND of the keys of workgroup g's tile (stores, no atomics: the plan kernel folds them in the next launch)
__global__ __launch_bounds__(MW_THREADS) void mw_key_bits_kernel(const u64* __restrict__ keys, WeldTiling t, u64* __restrict__ or_and) {
    __shared__ u64 lds[MW_WAVES][2];
    const u64 start = (u64)blockIdx.x * t.tile, end = min((u64)t.S, start + t.tile);
    u64 o = 0ull, a = ~0ull;
    for (u64 i = start + threadIdx.x; i < end; i += MW_THREADS) {
        const u64 k = keys[i];
        o |= k;
        a &= k;
    }
    block_or_and(o, a, lds);
    if (threadIdx.x == 0u) {
        or_and[2u * blockIdx.x] = o;
        or_and[2u * blockIdx.x + 1u] = a;
    }
}

// One workgroup: folds the tiles' words, then one thread marks the passes whose digit differs somewhere and deals them the buffers they read and write
__global__ __launch_bounds__(MW_THREADS) void mw_plan_kernel(const u64* __restrict__ or_and, u32 workgroups, u32* __restrict__ counters) {
    __shared__ u64 lds[MW_WAVES][2];
    u64 o = 0ull, a = ~0ull;
    for (u32 g = threadIdx.x; g < workgroups; g += MW_THREADS) {
        o |= or_and[2u * g];
        a &= or_and[2u * g + 1u];
    }
    block_or_and(o, a, lds);
    if (threadIdx.x != 0u) return;
    const u64 differs = o ^ a;
    u32 cur = 0u, n = 0u;
    for (u32 p = 0; p < MW_PASSES; p++) {
        const bool run = ((differs >> (p * MW_RADIX_BITS)) & (u64)(MW_RADIX - 1u)) != 0ull;
        const u32 out = run ? (cur == 1u ? 2u : 1u) : cur;
        counters[MW_C_RUN + p] = run ? 1u : 0u;
        counters[MW_C_IN + p] = cur;
        counters[MW_C_OUT + p] = out;
        cur = out;
        n += run ? 1u : 0u;
    }
    counters[MW_C_PASSES] = n;
    counters[MW_C_FINAL] = cur;
}

// table[d * workgroups + g] = the number of keys of workgroup g's tile with digit d.  LDS integer atomics; a wave whose 64 keys share the digit (the high
// digits of keys that arrive nearly sorted, as the TSDF's do) adds once.
__global__ __launch_bounds__(MW_THREADS) void mw_histogram_kernel(u32 pass, WeldBuffers b, WeldTiling t, const u32* __restrict__ counters, u32* __restrict__ table) {
    if (counters[MW_C_RUN + pass] == 0u) return;
    __shared__ u32 hist[MW_RADIX];
    const u64* __restrict__ keys = b.keys_of(counters[MW_C_IN + pass]);
    const u32 lane = threadIdx.x & 63u;
    hist[threadIdx.x] = 0u;
    __syncthreads();
    const u64 start = (u64)blockIdx.x * t.tile, end = min((u64)t.S, start + t.tile);
    for (u64 base = start; base < end; base += MW_THREADS) {
        const u64 i = base + threadIdx.x;
        const bool valid = i < end;
        const u32 d = valid ? digit_of(keys[i], pass) : 0u;
        const u64 vm = __ballot(valid);
        if (vm == 0ull) continue;   // (uniform in the wave; no barrier inside the loop)
        const u32 lead = (u32)(__ffsll((long long)vm) - 1);
        const u32 d0 = (u32)__shfl((int)d, (int)lead, 64);
        if (__ballot(valid && d != d0) == 0ull) {
            if (lane == lead) atomicAdd(&hist[d0], (u32)__popcll(vm));
        } else if (valid) {
            atomicAdd(&hist[d], 1u);
        }
    }
    __syncthreads();
    table[(size_t)threadIdx.x * t.workgroups + blockIdx.x] = hist[threadIdx.x];
}

// The stable scatter.  offsets: the exclusive scan of the histogram's table, so offsets[d * workgroups + g] is where workgroup g's first pair of digit d goes.
// The workgroup walks its tile in subtiles of 4096 pairs, in order; inside a subtile wave w holds pairs [w * 1024, (w + 1) * 1024) as 16 chunks of 64 in
// registers.  Count: per chunk the lanes of equal digit find each other by ballots, the pair's place among its wave's pairs of that digit is (what the wave
// counted in earlier chunks) + (equal lanes below), and the group's lowest lane adds the group's size to the wave's count -- a row of LDS only this wave
// touches, in program order.  Between two barriers thread d turns the four waves' counts of digit d into the waves' bases, running on from the subtile before.
// Scatter: pair -> base of (wave, digit) + place.  Order within a digit is subtile, wave, chunk, lane: ascending input index.
__global__ __launch_bounds__(MW_THREADS) void mw_scatter_kernel(u32 pass, WeldBuffers b, WeldTiling t, const u32* __restrict__ counters, const u32* __restrict__ offsets) {
    if (counters[MW_C_RUN + pass] == 0u) return;
    __shared__ u32 wave_counts[MW_WAVES][MW_RADIX];
    __shared__ u32 digit_base[MW_RADIX];
    const u32 in = counters[MW_C_IN + pass], out = counters[MW_C_OUT + pass];
    const u64* __restrict__ keys_in = b.keys_of(in);
    const u32* __restrict__ slots_in = b.slots_of(in);
    u64* __restrict__ keys_out = b.keys[out - 1u];   // (a pass that runs writes buffer 1 or 2)
    u32* __restrict__ slots_out = b.slots[out - 1u];
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    volatile u32* mine = wave_counts[wave];
    digit_base[threadIdx.x] = offsets[(size_t)threadIdx.x * t.workgroups + blockIdx.x];
    const u64 start = (u64)blockIdx.x * t.tile, end = min((u64)t.S, start + t.tile);
    for (u64 sub = start; sub < end; sub += MW_SUBTILE) {   // (uniform in the workgroup)
#pragma unroll
        for (u32 w = 0; w < MW_WAVES; w++) wave_counts[w][threadIdx.x] = 0u;
        __syncthreads();
        const u64 first = sub + (u64)wave * (MW_CHUNKS * 64u) + lane;
        u64 key[MW_CHUNKS];
        u32 slot[MW_CHUNKS], place[MW_CHUNKS];
#pragma unroll
        for (u32 c = 0; c < MW_CHUNKS; c++) {
            const u64 i = first + c * 64u;
            const bool valid = i < end;
            key[c] = valid ? keys_in[i] : 0ull;
            slot[c] = valid ? (slots_in ? slots_in[i] : (u32)i) : 0u;
        }
#pragma unroll
        for (u32 c = 0; c < MW_CHUNKS; c++) {
            const bool valid = first + c * 64u < end;
            const u32 d = digit_of(key[c], pass);
            const u64 vm = __ballot(valid);
            u64 m = vm;
            if (vm != 0ull) {
                const u32 d0 = (u32)__shfl((int)d, __ffsll((long long)vm) - 1, 64);
                if (__ballot(valid && d != d0) != 0ull) m = match_digit<MW_RADIX_BITS>(d, vm);
            }
            const u32 rank = lanes_below(m);
            u32 before = 0u;
            if (valid) before = mine[d];
            if (valid && rank == 0u) mine[d] = before + (u32)__popcll(m);
            place[c] = before + rank;
        }
        __syncthreads();
        {
            u32 run = digit_base[threadIdx.x];
#pragma unroll
            for (u32 w = 0; w < MW_WAVES; w++) {
                const u32 n = wave_counts[w][threadIdx.x];
                wave_counts[w][threadIdx.x] = run;
                run += n;
            }
            digit_base[threadIdx.x] = run;
        }
        __syncthreads();
#pragma unroll
        for (u32 c = 0; c < MW_CHUNKS; c++) {
            if (first + c * 64u < end) {
                const u32 dst = mine[digit_of(key[c], pass)] + place[c];
                keys_out[dst] = key[c];
                slots_out[dst] = slot[c];
            }
        }
        __syncthreads();
    }
}

// flags[i] = 1 where sorted pair i begins a run of equal keys
__global__ __launch_bounds__(MW_THREADS) void mw_heads_kernel(WeldBuffers b, u32 S, const u32* __restrict__ counters, u32* __restrict__ flags) {
    const u64 i = (u64)blockIdx.x * MW_THREADS + threadIdx.x;
    if (i >= S) return;
    const u64* __restrict__ keys = b.keys_of(counters[MW_C_FINAL]);
    flags[i] = (i == 0ull || keys[i] != keys[i - 1ull]) ? 1u : 0u;
}

// ids: the exclusive scan of flags, so pair i belongs to vertex ids[i] + flags[i] - 1.  faces[slot] = that vertex; a head also writes its vertex: the key, and the
// position and colour of its slot (each of the three outputs nullable).
__global__ __launch_bounds__(MW_THREADS) void mw_emit_kernel(WeldBuffers b, u32 S, const u32* __restrict__ counters, const u32* __restrict__ flags, const u32* __restrict__ ids,
                                                             const float* __restrict__ positions, const u32* __restrict__ colours, u64* __restrict__ keys_out,
                                                             float* __restrict__ vertices_out, u32* __restrict__ colours_out, u32* __restrict__ faces_out) {
    const u64 i = (u64)blockIdx.x * MW_THREADS + threadIdx.x;
    if (i >= S) return;
    const u32 final_buffer = counters[MW_C_FINAL];
    const u32* __restrict__ slots = b.slots_of(final_buffer);
    const u32 slot = slots ? slots[i] : (u32)i;
    const u32 head = flags[i], v = ids[i] + head - 1u;
    faces_out[slot] = v;
    if (head == 0u) return;
    if (keys_out) keys_out[v] = b.keys_of(final_buffer)[i];
    if (vertices_out) {
#pragma unroll
        for (u32 a = 0; a < 3u; a++) vertices_out[3u * (size_t)v + a] = positions[3u * (size_t)slot + a];
    }
    if (colours_out) colours_out[v] = colours[slot];
}

WeldTiling weld_tiling(u32 S) {
    const u32 per = ceil_div(S, MW_MAX_WORKGROUPS);
    const u32 tile = std::max(MW_SUBTILE, ceil_div(per, MW_SUBTILE) * MW_SUBTILE);
    return WeldTiling{S, tile, ceil_div(S, tile)};
}

inline dim3 per_slot_grid(u32 S) { return dim3((u32)(((u64)S + MW_THREADS - 1u) / MW_THREADS)); }

}  // namespace

// ---------------------------------------------------------------- launchers
int launch_weld_plan(wdgs_device* dev, const unsigned long long* keys, u32 S, unsigned long long* or_and, u32* counters) {
    const WeldTiling t = weld_tiling(S);
    WDGS_LAUNCH(dev, "weld_key_bits", mw_key_bits_kernel, dim3(t.workgroups), dim3(MW_THREADS), 0, keys, t, or_and);
    WDGS_LAUNCH(dev, "weld_plan", mw_plan_kernel, dim3(1), dim3(MW_THREADS), 0, (const u64*)or_and, t.workgroups, counters);
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

u32 weld_table_words(u32 S) { return S == 0u ? 0u : MW_RADIX * weld_tiling(S).workgroups; }

int launch_weld_sort(wdgs_device* dev, ScanScratch* scan, const unsigned long long* keys, u32 S, unsigned long long* keys_a, unsigned long long* keys_b, u32* slots_a,
                     u32* slots_b, const u32* counters, u32* table, u32* offsets) {
    const WeldTiling t = weld_tiling(S);
    const WeldBuffers b{keys, {keys_a, keys_b}, {slots_a, slots_b}};
    for (u32 pass = 0; pass < MW_PASSES; pass++) {
        WDGS_LAUNCH(dev, "weld_histogram", mw_histogram_kernel, dim3(t.workgroups), dim3(MW_THREADS), 0, pass, b, t, counters, table);
        WDGS_TRY(scan_exclusive_u32(dev, scan, table, offsets, MW_RADIX * t.workgroups, nullptr));
        WDGS_LAUNCH(dev, "weld_scatter", mw_scatter_kernel, dim3(t.workgroups), dim3(MW_THREADS), 0, pass, b, t, counters, (const u32*)offsets);
    }
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

int launch_weld_heads(wdgs_device* dev, const unsigned long long* keys, u32 S, const unsigned long long* keys_a, const unsigned long long* keys_b, const u32* counters,
                      u32* flags) {
    const WeldBuffers b{keys, {const_cast<u64*>(keys_a), const_cast<u64*>(keys_b)}, {nullptr, nullptr}};
    WDGS_LAUNCH(dev, "weld_heads", mw_heads_kernel, per_slot_grid(S), dim3(MW_THREADS), 0, b, S, counters, flags);
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

int launch_weld_emit(wdgs_device* dev, const unsigned long long* keys, u32 S, const unsigned long long* keys_a, const unsigned long long* keys_b, const u32* slots_a,
                     const u32* slots_b, const u32* counters, const u32* flags, const u32* ids, const float* positions, const u32* colours, unsigned long long* keys_out,
                     float* vertices_out, u32* colours_out, u32* faces_out) {
    const WeldBuffers b{keys, {const_cast<u64*>(keys_a), const_cast<u64*>(keys_b)}, {const_cast<u32*>(slots_a), const_cast<u32*>(slots_b)}};
    WDGS_LAUNCH(dev, "weld_emit", mw_emit_kernel, per_slot_grid(S), dim3(MW_THREADS), 0, b, S, counters, flags, ids, positions, colours, keys_out, vertices_out, colours_out,
                faces_out);
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

// ---------------------------------------------------------------- the C ABI object (include/webdgs.h)
struct wdgs_mesh_welder {
    wdgs_device* dev = nullptr;
    DevMem<unsigned long long> keys_a, keys_b;   // [S]: the two pair buffers the passes alternate between
    DevMem<u32> slots_a, slots_b;                // [S]
    DevMem<u32> flags, ids;                      // [S]: the head flags of the sorted pairs and their scan
    DevMem<u32> table, offsets;                  // [256 * workgroups]: a pass's digit-major histogram and its scan
    DevMem<unsigned long long> or_and;           // [2 * workgroups]: the OR and the AND of every tile's keys
    DevMem<u32> counters;                        // MW_C_WORDS: V and the plan
    ScanScratch scan;
    u32 capacity_s = 0, capacity_table = 0, capacity_scan = 0;
    bool counted = false;
    const void* keys = nullptr;                  // the caller's, read again by emit when no pass ran
    u32 S = 0, V = 0, passes_run = 0;
};

extern "C" int wdgs_mesh_welder_create(wdgs_device* dev, wdgs_mesh_welder** out) {
    WDGS_REQUIRE(dev && out, WDGS_E_INVALID, "wdgs_mesh_welder_create: null argument");
    WDGS_REQUIRE(!dev->capturing, WDGS_E_STATE, "wdgs_mesh_welder_create while recording a command buffer");
    auto w = std::make_unique<wdgs_mesh_welder>();
    w->dev = dev;
    WDGS_TRY(w->counters.alloc(MW_C_WORDS, true, dev->stream));
    *out = w.release();
    return WDGS_OK;
}

extern "C" int wdgs_mesh_welder_destroy(wdgs_mesh_welder* w) {
    if (!w) return WDGS_OK;
    if (wdgs_device_alive(w->dev) && !w->dev->capturing) (void)wdgs_sync_lanes(w->dev);
    delete w;
    return WDGS_OK;
}

extern "C" int wdgs_mesh_welder_count(wdgs_mesh_welder* w, const void* keys_u64_dev, uint64_t num_slots, uint32_t* num_vertices) {
    WDGS_REQUIRE(w && num_vertices, WDGS_E_INVALID, "wdgs_mesh_welder_count: null argument");
    w->counted = false;   // (a refused count leaves nothing to emit)
    WDGS_REQUIRE(num_slots < (1ull << 32) && num_slots % 3ull == 0ull, WDGS_E_INVALID, "weldTriangles: %llu slots: not three per triangle, or 2^32 or more",
                 (unsigned long long)num_slots);
    WDGS_REQUIRE(num_slots == 0 || keys_u64_dev, WDGS_E_INVALID, "wdgs_mesh_welder_count: null keys");
    WDGS_REQUIRE(((uintptr_t)keys_u64_dev & 7u) == 0u, WDGS_E_INVALID, "wdgs_mesh_welder_count: misaligned keys");
    wdgs_device* d = w->dev;
    WDGS_REQUIRE(!d->capturing, WDGS_E_STATE, "weldTriangles: the count waits for its vertex count and cannot be recorded into a command buffer");
    *num_vertices = 0;
    const u32 S = (u32)num_slots;
    const u32 table_words = weld_table_words(S);
    if (S > w->capacity_s || table_words > w->capacity_table || std::max(S, table_words) > w->capacity_scan) {
        WDGS_CHECK_HIP(wdgs_sync_lanes(d));   // (nothing in flight may still read the blocks given back)
        if (S > w->capacity_s) {
            w->capacity_s = 0;
            WDGS_TRY(w->keys_a.alloc(S, false, d->stream));
            WDGS_TRY(w->keys_b.alloc(S, false, d->stream));
            WDGS_TRY(w->slots_a.alloc(S, false, d->stream));
            WDGS_TRY(w->slots_b.alloc(S, false, d->stream));
            WDGS_TRY(w->flags.alloc(S, false, d->stream));
            WDGS_TRY(w->ids.alloc(S, false, d->stream));
            w->capacity_s = S;
        }
        if (table_words > w->capacity_table) {
            w->capacity_table = 0;
            WDGS_TRY(w->table.alloc(table_words, false, d->stream));
            WDGS_TRY(w->offsets.alloc(table_words, false, d->stream));
            WDGS_TRY(w->or_and.alloc(2u * (table_words / 256u), false, d->stream));
            w->capacity_table = table_words;
        }
        if (std::max(S, table_words) > w->capacity_scan) {
            w->capacity_scan = 0;
            WDGS_TRY(scan_scratch_create(&w->scan, std::max(S, table_words)));
            w->capacity_scan = std::max(S, table_words);
        }
    }
    u32 host[3] = {0u, 0u, 0u};
    if (S != 0) {
        const unsigned long long* keys = static_cast<const unsigned long long*>(keys_u64_dev);
        WDGS_TRY(launch_weld_plan(d, keys, S, w->or_and, w->counters));
        WDGS_TRY(launch_weld_sort(d, &w->scan, keys, S, w->keys_a, w->keys_b, w->slots_a, w->slots_b, w->counters, w->table, w->offsets));
        WDGS_TRY(launch_weld_heads(d, keys, S, w->keys_a, w->keys_b, w->counters, w->flags));
        WDGS_TRY(scan_exclusive_u32(d, &w->scan, w->flags, w->ids, S, w->counters + MW_C_TOTAL));
        WDGS_CHECK_HIP(hipMemcpyAsync(host, w->counters, sizeof(host), hipMemcpyDeviceToHost, d->stream));
        WDGS_CHECK_HIP(wdgs_sync_lanes(d));
    }
    w->keys = keys_u64_dev;
    w->S = S;
    w->V = host[MW_C_TOTAL];
    w->passes_run = host[MW_C_PASSES];
    w->counted = true;
    *num_vertices = w->V;
    return WDGS_OK;
}

extern "C" int wdgs_mesh_welder_emit(wdgs_mesh_welder* w, const void* keys_u64_dev, uint64_t num_slots, const void* positions_f32_dev, const void* colours_rgba8_dev,
                                     void* keys_out_u64_dev, void* vertices_out_f32_dev, void* colours_out_rgba8_dev, void* faces_out_u32_dev, uint32_t capacity_vertices) {
    WDGS_REQUIRE(w, WDGS_E_INVALID, "wdgs_mesh_welder_emit: null argument");
    WDGS_REQUIRE(w->counted && keys_u64_dev == w->keys && num_slots == (uint64_t)w->S, WDGS_E_STATE, "weldTriangles: no count of these keys precedes the emit");
    WDGS_REQUIRE(capacity_vertices >= w->V, WDGS_E_CAPACITY, "weldTriangles: %u vertices, room for %u", w->V, capacity_vertices);
    WDGS_REQUIRE((positions_f32_dev == nullptr) == (vertices_out_f32_dev == nullptr), WDGS_E_INVALID, "wdgs_mesh_welder_emit: positions need both an input and an output");
    WDGS_REQUIRE((colours_rgba8_dev == nullptr) == (colours_out_rgba8_dev == nullptr), WDGS_E_INVALID, "wdgs_mesh_welder_emit: colours need both an input and an output");
    WDGS_REQUIRE(w->S == 0 || faces_out_u32_dev, WDGS_E_INVALID, "wdgs_mesh_welder_emit: null faces output");
    WDGS_REQUIRE((((uintptr_t)positions_f32_dev | (uintptr_t)colours_rgba8_dev | (uintptr_t)vertices_out_f32_dev | (uintptr_t)colours_out_rgba8_dev | (uintptr_t)faces_out_u32_dev) & 3u) == 0u &&
                     ((uintptr_t)keys_out_u64_dev & 7u) == 0u,
                 WDGS_E_INVALID, "wdgs_mesh_welder_emit: misaligned buffer");
    if (w->S == 0) return WDGS_OK;
    return launch_weld_emit(w->dev, static_cast<const unsigned long long*>(keys_u64_dev), w->S, w->keys_a, w->keys_b, w->slots_a, w->slots_b, w->counters, w->flags, w->ids,
                            static_cast<const float*>(positions_f32_dev), static_cast<const u32*>(colours_rgba8_dev), static_cast<unsigned long long*>(keys_out_u64_dev),
                            static_cast<float*>(vertices_out_f32_dev), static_cast<u32*>(colours_out_rgba8_dev), static_cast<u32*>(faces_out_u32_dev));
}

extern "C" int wdgs_mesh_welder_stats(const wdgs_mesh_welder* w, uint32_t* passes_run, uint32_t* passes_skipped, uint32_t* num_vertices, uint32_t* num_slots) {
    WDGS_REQUIRE(w, WDGS_E_INVALID, "wdgs_mesh_welder_stats: null argument");
    WDGS_REQUIRE(w->counted, WDGS_E_STATE, "weldTriangles: no count precedes the read of its statistics");
    if (passes_run) *passes_run = w->passes_run;
    if (passes_skipped) *passes_skipped = MW_PASSES - w->passes_run;
    if (num_vertices) *num_vertices = w->V;
    if (num_slots) *num_slots = w->S;
    return WDGS_OK;
}
