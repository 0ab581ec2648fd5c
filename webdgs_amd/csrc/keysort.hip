// KeySort (launch.h): a stable sort of u64 keys on the device with what groups by a key wants of it -- the rank of every slot's key among the distinct keys,
// the distinct keys, and a payload gathered from the LOWEST slot that carries each.  Its users are the welder (meshweld.hip) and the
// simplifier's three sorts (meshsimplify.hip, section 18).
//
// The sort is an LSD radix sort of (key, slot) pairs by 8-bit digits.  Every pass is stable and the slots start ascending, so after the last pass equal keys
// lie together in ascending slot order and the head of a run is its lowest slot.  Everything is integer work and every output is a function of the input alone.
//
// No kernel here reads what another workgroup of the same launch writes, and there is no global atomic at all: every kernel reads what earlier launches wrote,
// with plain loads.  A pass is three launches -- histogram, the library's scan over the digit-major table, scatter -- and the order between workgroups comes
// from the scanned table alone: no workgroup waits for another, polls a flag or looks back at a neighbour's partial result.
//
// Which passes run is decided on the device: ks_key_bits leaves every tile's OR and AND of its keys, ks_plan folds them, marks the passes whose digit differs
// somewhere (a bit set in OR ^ AND) and deals them the buffers in turn (0 = the caller's keys with slot = index, 1 and 2 = the sort's pairs).  The kernels of
// a pass whose digit is the same in every key return at once, so the host never has to know the plan.
#include "keysort_sizes.h"
#include "launch.h"

namespace {

using namespace wdgs;
typedef unsigned long long u64;

constexpr u32 KS_WAVES = KS_THREADS / 64;
static_assert(KS_THREADS == KS_RADIX, "one thread per digit in the scatter's table phases");
static_assert(KS_PASSES == 64 / KS_RADIX_BITS, "launch.h's pass count is the key's digits");

__device__ __forceinline__ u32 digit_of(u64 key, u32 pass) { return (u32)(key >> (pass * KS_RADIX_BITS)) & (KS_RADIX - 1u); }

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
    for (u32 w = 0; w < KS_WAVES; w++) {
        o |= lds[w][0];
        a &= lds[w][1];
    }
}

// or_and[2 g], or_and[2 g + 1]: the OR and the AND of the keys of workgroup g's tile (stores, no atomics: the plan kernel folds them in the next launch)
__global__ __launch_bounds__(KS_THREADS) void ks_key_bits_kernel(const u64* __restrict__ keys, KeySortTiling t, u64* __restrict__ or_and) {
    __shared__ u64 lds[KS_WAVES][2];
    const u64 start = (u64)blockIdx.x * t.tile, end = min((u64)t.S, start + t.tile);
    u64 o = 0ull, a = ~0ull;
    for (u64 i = start + threadIdx.x; i < end; i += KS_THREADS) {
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
__global__ __launch_bounds__(KS_THREADS) void ks_plan_kernel(const u64* __restrict__ or_and, u32 workgroups, u32* __restrict__ counters) {
    __shared__ u64 lds[KS_WAVES][2];
    u64 o = 0ull, a = ~0ull;
    for (u32 g = threadIdx.x; g < workgroups; g += KS_THREADS) {
        o |= or_and[2u * g];
        a &= or_and[2u * g + 1u];
    }
    block_or_and(o, a, lds);
    if (threadIdx.x != 0u) return;
    const u64 differs = o ^ a;
    u32 cur = 0u, n = 0u;
    for (u32 p = 0; p < KS_PASSES; p++) {
        const bool run = ((differs >> (p * KS_RADIX_BITS)) & (u64)(KS_RADIX - 1u)) != 0ull;
        const u32 out = run ? (cur == 1u ? 2u : 1u) : cur;
        counters[KS_C_RUN + p] = run ? 1u : 0u;
        counters[KS_C_IN + p] = cur;
        counters[KS_C_OUT + p] = out;
        cur = out;
        n += run ? 1u : 0u;
    }
    counters[KS_C_PASSES] = n;
    counters[KS_C_FINAL] = cur;
}

// table[d * workgroups + g] = the number of keys of workgroup g's tile with digit d.  LDS integer atomics; a wave whose 64 keys share the digit (the high
// digits of keys that arrive nearly sorted, as the TSDF's do) adds once.
__global__ __launch_bounds__(KS_THREADS) void ks_histogram_kernel(u32 pass, KeySortView b, KeySortTiling t, const u32* __restrict__ counters, u32* __restrict__ table) {
    if (counters[KS_C_RUN + pass] == 0u) return;
    __shared__ u32 hist[KS_RADIX];
    const u64* __restrict__ keys = b.keys_of(counters[KS_C_IN + pass]);
    const u32 lane = threadIdx.x & 63u;
    hist[threadIdx.x] = 0u;
    __syncthreads();
    const u64 start = (u64)blockIdx.x * t.tile, end = min((u64)t.S, start + t.tile);
    for (u64 base = start; base < end; base += KS_THREADS) {
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
__global__ __launch_bounds__(KS_THREADS) void ks_scatter_kernel(u32 pass, KeySortView b, KeySortTiling t, const u32* __restrict__ counters, const u32* __restrict__ offsets) {
    if (counters[KS_C_RUN + pass] == 0u) return;
    __shared__ u32 wave_counts[KS_WAVES][KS_RADIX];
    __shared__ u32 digit_base[KS_RADIX];
    const u32 in = counters[KS_C_IN + pass], out = counters[KS_C_OUT + pass];
    const u64* __restrict__ keys_in = b.keys_of(in);
    const u32* __restrict__ slots_in = b.slots_of(in);
    u64* __restrict__ keys_out = b.keys[out - 1u];   // (a pass that runs writes buffer 1 or 2)
    u32* __restrict__ slots_out = b.slots[out - 1u];
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    volatile u32* mine = wave_counts[wave];
    digit_base[threadIdx.x] = offsets[(size_t)threadIdx.x * t.workgroups + blockIdx.x];
    const u64 start = (u64)blockIdx.x * t.tile, end = min((u64)t.S, start + t.tile);
    for (u64 sub = start; sub < end; sub += KS_SUBTILE) {   // (uniform in the workgroup)
#pragma unroll
        for (u32 w = 0; w < KS_WAVES; w++) wave_counts[w][threadIdx.x] = 0u;
        __syncthreads();
        const u64 first = sub + (u64)wave * (KS_CHUNKS * 64u) + lane;
        u64 key[KS_CHUNKS];
        u32 slot[KS_CHUNKS], place[KS_CHUNKS];
#pragma unroll
        for (u32 c = 0; c < KS_CHUNKS; c++) {
            const u64 i = first + c * 64u;
            const bool valid = i < end;
            key[c] = valid ? keys_in[i] : 0ull;
            slot[c] = valid ? (slots_in ? slots_in[i] : (u32)i) : 0u;
        }
#pragma unroll
        for (u32 c = 0; c < KS_CHUNKS; c++) {
            const bool valid = first + c * 64u < end;
            const u32 d = digit_of(key[c], pass);
            const u64 vm = __ballot(valid);
            u64 m = vm;
            if (vm != 0ull) {
                const u32 d0 = (u32)__shfl((int)d, __ffsll((long long)vm) - 1, 64);
                if (__ballot(valid && d != d0) != 0ull) m = match_digit<KS_RADIX_BITS>(d, vm);
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
            for (u32 w = 0; w < KS_WAVES; w++) {
                const u32 n = wave_counts[w][threadIdx.x];
                wave_counts[w][threadIdx.x] = run;
                run += n;
            }
            digit_base[threadIdx.x] = run;
        }
        __syncthreads();
#pragma unroll
        for (u32 c = 0; c < KS_CHUNKS; c++) {
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
__global__ __launch_bounds__(KS_THREADS) void ks_heads_kernel(KeySortView b, u32 S, const u32* __restrict__ counters, u32* __restrict__ flags) {
    const u64 i = (u64)blockIdx.x * KS_THREADS + threadIdx.x;
    if (i >= S) return;
    const u64* __restrict__ keys = b.keys_of(counters[KS_C_FINAL]);
    flags[i] = (i == 0ull || keys[i] != keys[i - 1ull]) ? 1u : 0u;
}

// ids: the exclusive scan of flags, so pair i carries distinct key number ids[i] + flags[i] - 1.  rank_out[slot] = that number; a head also writes what belongs to
// its key: the key, and the three floats and the word its slot has in the two payloads (each of the three outputs nullable).
__global__ __launch_bounds__(KS_THREADS) void ks_emit_kernel(KeySortView b, u32 S, const u32* __restrict__ counters, const u32* __restrict__ flags, const u32* __restrict__ ids,
                                                             const float* __restrict__ gather_f32x3, const u32* __restrict__ gather_u32, u64* __restrict__ keys_out,
                                                             float* __restrict__ gather_f32x3_out, u32* __restrict__ gather_u32_out, u32* __restrict__ rank_out) {
    const u64 i = (u64)blockIdx.x * KS_THREADS + threadIdx.x;
    if (i >= S) return;
    const u32 final_buffer = counters[KS_C_FINAL];
    const u32* __restrict__ slots = b.slots_of(final_buffer);
    const u32 slot = slots ? slots[i] : (u32)i;
    const u32 head = flags[i], v = ids[i] + head - 1u;
    rank_out[slot] = v;
    if (head == 0u) return;
    if (keys_out) keys_out[v] = b.keys_of(final_buffer)[i];
    if (gather_f32x3_out) {
#pragma unroll
        for (u32 a = 0; a < 3u; a++) gather_f32x3_out[3u * (size_t)v + a] = gather_f32x3[3u * (size_t)slot + a];
    }
    if (gather_u32_out) gather_u32_out[v] = gather_u32[slot];
}

inline dim3 per_slot_grid(u32 S) { return dim3((u32)(((u64)S + KS_THREADS - 1u) / KS_THREADS)); }

}  // namespace

int KeySort::create(wdgs_device* dev) { return counters.alloc(KS_C_WORDS, true, dev->stream); }

int KeySort::reserve(wdgs_device* dev, u32 S_a, u32 S_b) {
    const KeySortSizes need = keysort_reserve_sizes(S_a, S_b);
    if (need.n <= capacity_n && need.table_words <= capacity_table && need.scan_words <= capacity_scan) return WDGS_OK;
    WDGS_CHECK_HIP(wdgs_sync_lanes(dev));   // (nothing in flight may still read the blocks given back)
    if (need.n > capacity_n) {
        capacity_n = 0;
        WDGS_TRY(keys_a.alloc(need.n, false, dev->stream));
        WDGS_TRY(keys_b.alloc(need.n, false, dev->stream));
        WDGS_TRY(slots_a.alloc(need.n, false, dev->stream));
        WDGS_TRY(slots_b.alloc(need.n, false, dev->stream));
        WDGS_TRY(flags.alloc(need.n, false, dev->stream));
        WDGS_TRY(ids.alloc(need.n, false, dev->stream));
        capacity_n = need.n;
    }
    if (need.table_words > capacity_table) {
        capacity_table = 0;
        WDGS_TRY(table.alloc(need.table_words, false, dev->stream));
        WDGS_TRY(offsets.alloc(need.table_words, false, dev->stream));
        WDGS_TRY(or_and.alloc(2u * (need.table_words / KS_RADIX), false, dev->stream));
        capacity_table = need.table_words;
    }
    if (need.scan_words > capacity_scan) {
        capacity_scan = 0;
        WDGS_TRY(scan_scratch_create(&scratch, need.scan_words));
        capacity_scan = need.scan_words;
    }
    return WDGS_OK;
}

int KeySort::sort(wdgs_device* dev, const unsigned long long* keys, u32 S, u32* total_out) {
    const KeySortTiling t = keysort_tiling(S);
    const KeySortView b = view(keys);
    WDGS_LAUNCH(dev, "weld_key_bits", ks_key_bits_kernel, dim3(t.workgroups), dim3(KS_THREADS), 0, keys, t, or_and.get());
    WDGS_LAUNCH(dev, "weld_plan", ks_plan_kernel, dim3(1), dim3(KS_THREADS), 0, (const u64*)or_and, t.workgroups, counters.get());
    WDGS_CHECK_HIP(hipGetLastError());
    for (u32 pass = 0; pass < KS_PASSES; pass++) {
        WDGS_LAUNCH(dev, "weld_histogram", ks_histogram_kernel, dim3(t.workgroups), dim3(KS_THREADS), 0, pass, b, t, b.counters, table.get());
        WDGS_TRY(scan_exclusive_u32(dev, &scratch, table, offsets, KS_RADIX * t.workgroups, nullptr));
        WDGS_LAUNCH(dev, "weld_scatter", ks_scatter_kernel, dim3(t.workgroups), dim3(KS_THREADS), 0, pass, b, t, b.counters, (const u32*)offsets);
    }
    WDGS_CHECK_HIP(hipGetLastError());
    WDGS_LAUNCH(dev, "weld_heads", ks_heads_kernel, per_slot_grid(S), dim3(KS_THREADS), 0, b, S, b.counters, flags.get());
    WDGS_CHECK_HIP(hipGetLastError());
    return scan_exclusive_u32(dev, &scratch, flags, ids, S, total_out);
}

int KeySort::emit(wdgs_device* dev, const unsigned long long* keys, u32 S, u32* rank_out, unsigned long long* keys_out, const u32* gather_u32, u32* gather_u32_out,
                  const float* gather_f32x3, float* gather_f32x3_out) {
    const KeySortView b = view(keys);
    WDGS_LAUNCH(dev, "weld_emit", ks_emit_kernel, per_slot_grid(S), dim3(KS_THREADS), 0, b, S, b.counters, (const u32*)flags, (const u32*)ids, gather_f32x3, gather_u32,
                keys_out, gather_f32x3_out, gather_u32_out, rank_out);
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

int KeySort::rank(wdgs_device* dev, const unsigned long long* keys, u32 S, u32* total_out, u32* rank_out, unsigned long long* keys_out, const u32* gather_u32,
                  u32* gather_u32_out, const float* gather_f32x3, float* gather_f32x3_out) {
    WDGS_TRY(sort(dev, keys, S, total_out));
    return emit(dev, keys, S, rank_out, keys_out, gather_u32, gather_u32_out, gather_f32x3, gather_f32x3_out);
}
