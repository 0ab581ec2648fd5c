// Mesh accuracy metrics (no counterpart in the reference, which renders colour only): area-weighted sampling of a triangle mesh, a
// uniform-grid point index with exact nearest-point queries under a cutoff, and exact integer distance statistics; and on the same index (section 15) the
// k nearest points of a query and 3DGS's scale initialisation from them.
//
// Everything here is f32 in the order written (-ffp-contract=off, no FMA), square roots and quotients through wd_sqrt / wd_div, and every sum an integer:
// tests/geometry_ref.py restates the three pieces in numpy float32 and the GPU tests compare bytes.  The grid of the index is a speed choice only -- the
// query's definition never mentions it, and section 14 holds the argument that no rounding can make a result depend on the cell edge.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>

#include "dmath.h"
#include "launch.h"

namespace {

constexpr u32 NO_INDEX = 0xFFFFFFFFu;
constexpr u32 MAX_CELLS = 1u << 26;

__device__ __forceinline__ bool finite3(float x, float y, float z) {
    const float inf = __builtin_inff();
    return fabsf(x) < inf && fabsf(y) < inf && fabsf(z) < inf;   // (a NaN fails the comparison)
}

// ---------------------------------------------------------------- 1. sampling
__device__ __forceinline__ u32 mix32(u32 x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
__device__ __forceinline__ u32 sample_hash(u32 seed, u32 t, u32 k, u32 j) { return mix32((mix32(mix32(mix32(seed + 0x9E3779B9u) ^ t) + k)) ^ (j * 0x85EBCA6Bu + 1u)); }
// ((h >> 9) + 1/2) 2^-23: exact, strictly inside (0, 1)
__device__ __forceinline__ float unit_float(u32 h) { return ((float)(h >> 9) + 0.5f) * 1.1920928955078125e-07f; }

// One thread per triangle: counts[t] = floor(area density + dither), 0 for a face that names a vertex >= V or whose product is not finite; the workgroup's
// sum is added to *total with one u64 atomic.
__global__ __launch_bounds__(256) void sample_count_kernel(const float* __restrict__ vertices, u32 V, const u32* __restrict__ faces, u32 F, float density, u32 seed,
                                                           u32* __restrict__ counts, unsigned long long* __restrict__ total) {
    __shared__ unsigned long long s_w[4];
    const u32 t = blockIdx.x * 256u + threadIdx.x;
    u32 n = 0u;
    if (t < F) {
        const u32 ia = faces[3u * (size_t)t], ib = faces[3u * (size_t)t + 1u], ic = faces[3u * (size_t)t + 2u];
        if (ia < V && ib < V && ic < V) {
            const float* A = vertices + 3u * (size_t)ia;
            const float* B = vertices + 3u * (size_t)ib;
            const float* C = vertices + 3u * (size_t)ic;
            const float e1x = B[0] - A[0], e1y = B[1] - A[1], e1z = B[2] - A[2];
            const float e2x = C[0] - A[0], e2y = C[1] - A[1], e2z = C[2] - A[2];
            const float nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
            const float area = 0.5f * wd_sqrt((nx * nx + ny * ny) + nz * nz);
            const float x = area * density + unit_float(sample_hash(seed, t, 0xFFFFFFFFu, 0u));
            if (fabsf(x) < __builtin_inff()) n = min(wd_to_u32(floorf(x)), 0x7FFFFFFFu);
        }
        counts[t] = n;
    }
    unsigned long long acc = n;
#pragma unroll
    for (u32 d = 32; d >= 1; d >>= 1) acc += (unsigned long long)__shfl_xor((long long)acc, (int)d, 64);
    if ((threadIdx.x & 63u) == 0u) s_w[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long s = s_w[0] + s_w[1] + s_w[2] + s_w[3];
        if (s) atomicAdd(total, s);
    }
}

// One thread per SAMPLE: its triangle is the last t with offsets[t] <= s (a triangle without samples shares its offset with its successor and is never that
// one), found by bisection, so a triangle of any size costs its samples and no more.  Sample k of triangle t lands at offsets[t] + k = s.
__global__ __launch_bounds__(256) void sample_emit_kernel(const float* __restrict__ vertices, u32 V, const u32* __restrict__ faces, u32 F, u32 seed,
                                                          const u32* __restrict__ offsets, u32 total, float* __restrict__ points, u32* __restrict__ face_out) {
    const u32 s = blockIdx.x * 256u + threadIdx.x;
    if (s >= total) return;
    u32 lo = 0u, hi = F;
    while (hi - lo > 1u) {
        const u32 mid = lo + ((hi - lo) >> 1);
        if (offsets[mid] <= s) lo = mid;
        else hi = mid;
    }
    const u32 t = lo, k = s - offsets[t];
    const u32 ia = faces[3u * (size_t)t], ib = faces[3u * (size_t)t + 1u], ic = faces[3u * (size_t)t + 2u];
    float* p = points + 3u * (size_t)s;
    if (face_out) face_out[s] = t;
    // (faces rewritten behind the library's back since the count may name any vertex now: nothing outside the vertex array is read)
    if (!(ia < V && ib < V && ic < V)) {
        p[0] = p[1] = p[2] = __builtin_nanf("");
        return;
    }
    float u = unit_float(sample_hash(seed, t, k, 1u)), v = unit_float(sample_hash(seed, t, k, 2u));
    if (u + v > 1.0f) { u = 1.0f - u; v = 1.0f - v; }
    const float* A = vertices + 3u * (size_t)ia;
    const float* B = vertices + 3u * (size_t)ib;
    const float* C = vertices + 3u * (size_t)ic;
#pragma unroll
    for (u32 a = 0; a < 3u; a++) {
        const float e1 = B[a] - A[a], e2 = C[a] - A[a];
        p[a] = (A[a] + u * e1) + v * e2;
    }
}

// ---------------------------------------------------------------- 2. the point index
struct PointGrid {
    float lox, loy, loz, cell;
    u32 nx, ny, nz;
    float slack;   // an upper bound on how far, in world units, a coordinate's computed cell can lie from its cell in exact arithmetic, times two (section 14)
};

// f32 bits in an order unsigned integers keep: negative numbers reversed below the positive ones
__device__ __forceinline__ u32 ordered_bits(float f) {
    const u32 b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
static float from_ordered_bits(u32 k) {
    const u32 b = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
    float f;
    memcpy(&f, &b, 4);
    return f;
}

// bounds: u32[7] = { min x, y, z, max x, y, z (ordered bits), finite points }; integer atomics, one set per workgroup
__global__ __launch_bounds__(256) void point_bounds_kernel(const float* __restrict__ points, u32 M, u32* __restrict__ bounds) {
    __shared__ u32 s_w[7][4];
    u32 mn[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, mx[3] = {0u, 0u, 0u}, cnt = 0u;
    for (u32 i = blockIdx.x * 256u + threadIdx.x; i < M; i += gridDim.x * 256u) {
        const float x = points[3u * (size_t)i], y = points[3u * (size_t)i + 1u], z = points[3u * (size_t)i + 2u];
        if (!finite3(x, y, z)) continue;
        const u32 kx = ordered_bits(x), ky = ordered_bits(y), kz = ordered_bits(z);
        mn[0] = min(mn[0], kx); mn[1] = min(mn[1], ky); mn[2] = min(mn[2], kz);
        mx[0] = max(mx[0], kx); mx[1] = max(mx[1], ky); mx[2] = max(mx[2], kz);
        cnt++;
    }
#pragma unroll
    for (u32 d = 32; d >= 1; d >>= 1) {
#pragma unroll
        for (u32 a = 0; a < 3u; a++) {
            mn[a] = min(mn[a], (u32)__shfl_xor((int)mn[a], (int)d, 64));
            mx[a] = max(mx[a], (u32)__shfl_xor((int)mx[a], (int)d, 64));
        }
        cnt += (u32)__shfl_xor((int)cnt, (int)d, 64);
    }
    const u32 w = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) {
        s_w[0][w] = mn[0]; s_w[1][w] = mn[1]; s_w[2][w] = mn[2];
        s_w[3][w] = mx[0]; s_w[4][w] = mx[1]; s_w[5][w] = mx[2];
        s_w[6][w] = cnt;
    }
    __syncthreads();
    if (threadIdx.x < 7u) {
        const u32* r = s_w[threadIdx.x];
        if (threadIdx.x < 3u) atomicMin(bounds + threadIdx.x, min(min(r[0], r[1]), min(r[2], r[3])));
        else if (threadIdx.x < 6u) atomicMax(bounds + threadIdx.x, max(max(r[0], r[1]), max(r[2], r[3])));
        else if (r[0] + r[1] + r[2] + r[3]) atomicAdd(bounds + 6, r[0] + r[1] + r[2] + r[3]);
    }
}

// The cell of a coordinate along one axis: floor((x - lo) / cell) clamped to [0, n - 1].  Each step is monotone in x (an f32 difference, an f32 quotient by a
// positive number, floor and the clamps all are), so the whole is: x <= y gives cell(x) <= cell(y), roundings and clamps included.  x may be +-inf.
__device__ __forceinline__ u32 cell_coord(float x, float lo, float cell, u32 n) {
    float f = floorf(wd_div(x - lo, cell));
    f = fmaxf(f, 0.0f);
    f = fminf(f, (float)(n - 1u));   // n <= 2^26: exact
    return (u32)f;
}

// cell_of[i]: the linear cell of point i (x fastest), rank[i]: its arrival number there (an integer atomic: any arrival order serves, see nearest_kernel).
// A non-finite point gets NO_INDEX and is counted nowhere, unless keep_all (the queries: they only need SOME place in the processing order): then cell 0.
__global__ __launch_bounds__(256) void point_cell_kernel(PointGrid g, const float* __restrict__ points, u32 n, u32 keep_all, u32* __restrict__ cell_of, u32* __restrict__ rank,
                                                         u32* __restrict__ counts) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float x = points[3u * (size_t)i], y = points[3u * (size_t)i + 1u], z = points[3u * (size_t)i + 2u];
    u32 c = NO_INDEX;
    if (finite3(x, y, z)) c = (cell_coord(z, g.loz, g.cell, g.nz) * g.ny + cell_coord(y, g.loy, g.cell, g.ny)) * g.nx + cell_coord(x, g.lox, g.cell, g.nx);
    else if (keep_all) c = 0u;
    cell_of[i] = c;
    if (c != NO_INDEX) rank[i] = atomicAdd(counts + c, 1u);
}

// records[starts[cell] + rank] = { x, y, z, original index }: the cell-sorted copy a query reads as whole 16-byte elements of consecutive addresses
__global__ __launch_bounds__(256) void point_scatter_kernel(const float* __restrict__ points, u32 n, const u32* __restrict__ cell_of, const u32* __restrict__ rank,
                                                            const u32* __restrict__ starts, float4* __restrict__ records) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const u32 c = cell_of[i];
    if (c == NO_INDEX) return;
    records[starts[c] + rank[i]] = make_float4(points[3u * (size_t)i], points[3u * (size_t)i + 1u], points[3u * (size_t)i + 2u], __uint_as_float(i));
}

// order[starts[cell] + rank] = i: the queries in cell order
__global__ __launch_bounds__(256) void query_order_kernel(u32 n, const u32* __restrict__ cell_of, const u32* __restrict__ rank, const u32* __restrict__ starts,
                                                          u32* __restrict__ order) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    order[starts[cell_of[i]] + rank[i]] = i;
}

// The running best of a query is a policy of nearest_kernel.  start() is the state of a query that finds nothing; search(r2) opens it for candidates --
// every place then holds { r2, NO_INDEX }, so the cutoff "d2 <= r2", the tie rule and "not yet full" are one comparison, whatever order the records come
// in; offer() is one candidate; worst() is what the early exit compares; finish() and write() close the search and store the query's row.
struct Best {
    struct Args {};
    float d2;
    u32 index;
    __device__ __forceinline__ void start(u32, Args) { d2 = __builtin_inff(); index = NO_INDEX; }
    __device__ __forceinline__ void search(float r2) { d2 = r2; }
    // kept when smaller, or equal with a lower original index
    __device__ __forceinline__ void offer(float c, u32 j) {
        const bool take = (c < d2) | ((c == d2) & (j < index));
        d2 = take ? c : d2;
        index = take ? j : index;
    }
    __device__ __forceinline__ float worst() const { return d2; }
    __device__ __forceinline__ void finish() { if (index == NO_INDEX) d2 = __builtin_inff(); }
    __device__ __forceinline__ void write(u32 q, float* __restrict__ d2_out, u32* __restrict__ index_out) const {
        d2_out[q] = d2;
        index_out[q] = index;
    }
};

// The k nearest (section 15): CAP slots in registers, sorted ascending by (d2, index).  The first CAP - k slots hold { -1, 0 }, which sorts before every
// candidate (d2 >= 0) and never moves, so the k-th nearest so far is always slot CAP - 1, a compile-time place.  `self`: the original index left out
// (NO_INDEX, which no record carries, leaves nothing out).  Every slot access is unrolled: nothing is indexed dynamically and nothing goes to scratch.
template <u32 CAP>
struct BestK {
    struct Args { u32 k, exclude_self; };
    float d2[CAP];
    u32 index[CAP];
    u32 k, self;
    __device__ __forceinline__ bool live(u32 s) const { return s + k >= CAP; }
    __device__ __forceinline__ void start(u32 q, Args a) {
        k = a.k;
        self = a.exclude_self ? q : NO_INDEX;
#pragma unroll
        for (u32 s = 0; s < CAP; s++) {
            d2[s] = live(s) ? __builtin_inff() : -1.0f;
            index[s] = live(s) ? NO_INDEX : 0u;
        }
    }
    __device__ __forceinline__ void search(float r2) {
#pragma unroll
        for (u32 s = 0; s < CAP; s++) d2[s] = live(s) ? r2 : d2[s];
    }
    // The excluded record fails before the comparison: it never enters the list and so never lets the search end early.  A candidate that beats the worst
    // replaces it and sinks to its place by CAP - 1 compare-and-swap steps of selects.
    __device__ __forceinline__ void offer(float c, u32 j) {
        const bool take = (j != self) & ((c < d2[CAP - 1u]) | ((c == d2[CAP - 1u]) & (j < index[CAP - 1u])));
        if (take) {
            d2[CAP - 1u] = c;
            index[CAP - 1u] = j;
#pragma unroll
            for (u32 s = CAP - 1u; s >= 1u; s--) {
                const float a = d2[s - 1u], b = d2[s];
                const u32 ia = index[s - 1u], ib = index[s];
                const bool swap = (b < a) | ((b == a) & (ib < ia));
                d2[s - 1u] = swap ? b : a;
                index[s - 1u] = swap ? ib : ia;
                d2[s] = swap ? a : b;
                index[s] = swap ? ia : ib;
            }
        }
    }
    __device__ __forceinline__ float worst() const { return d2[CAP - 1u]; }
    __device__ __forceinline__ void finish() {
#pragma unroll
        for (u32 s = 0; s < CAP; s++) d2[s] = index[s] == NO_INDEX ? __builtin_inff() : d2[s];
    }
    // row q of [K][k]: the live slots in order
    __device__ __forceinline__ void write(u32 q, float* __restrict__ d2_out, u32* __restrict__ index_out) const {
        float* d2_row = d2_out + (size_t)q * k;
        u32* index_row = index_out + (size_t)q * k;
#pragma unroll
        for (u32 s = 0; s < CAP; s++) {
            if (live(s)) {
                d2_row[s + k - CAP] = d2[s];
                index_row[s + k - CAP] = index[s];
            }
        }
    }
};

// One record against the query: d2 = ((dx dx + dy dy) + dz dz), offered to the running best.
template <class B>
__device__ __forceinline__ void test_record(const float4 r, float px, float py, float pz, B& best) {
    const float dx = px - r.x, dy = py - r.y, dz = pz - r.z;
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    best.offer(d2, __float_as_uint(r.w));
}
// The records [first, last) against the query, four 16-byte loads in flight at a time: the loop is bound by its arithmetic, not by one load's latency.
template <class B>
__device__ __forceinline__ void scan_records(const float4* __restrict__ records, u32 first, u32 last, float px, float py, float pz, B& best) {
    u32 i = first;
    for (; i + 4u <= last; i += 4u) {
        const float4 r0 = records[i], r1 = records[i + 1u], r2 = records[i + 2u], r3 = records[i + 3u];
        test_record(r0, px, py, pz, best);
        test_record(r1, px, py, pz, best);
        test_record(r2, px, py, pz, best);
        test_record(r3, px, py, pz, best);
    }
    for (; i < last; i++) test_record(records[i], px, py, pz, best);
}

// One thread per query, the queries taken in cell order (a wave's 64 queries walk the same few cells).  The cells searched are, per axis, those from
// cell(p - R) to cell(p + R), R a little above the cutoff: every point with d2 <= r2 lies in them (section 14: cell() is monotone).  They are visited in rings
// of growing Chebyshev distance k from the query's own cell; after ring k every unvisited point is farther than T_k = (k cell - slack) 0.9999, and the search
// ends once best.worst() < T_k^2 STRICTLY -- a point of an outer ring with the same d2 and a lower index must still be seen.  B: Best for the nearest point,
// BestK<CAP> for the k nearest (section 15) -- one walk, two ways of keeping what it finds.
template <class B, bool COUNT>
__global__ __launch_bounds__(256) void nearest_kernel(PointGrid g, const float4* __restrict__ records, const u32* __restrict__ starts, const float* __restrict__ queries,
                                                      const u32* __restrict__ order, u32 K, float r, float r2, float* __restrict__ d2_out, u32* __restrict__ index_out,
                                                      unsigned long long* __restrict__ pairs, typename B::Args args) {
    const u32 tid = blockIdx.x * 256u + threadIdx.x;
    unsigned long long examined = 0ull;
    if (tid < K) {
        const u32 q = order[tid];
        const float px = queries[3u * (size_t)q], py = queries[3u * (size_t)q + 1u], pz = queries[3u * (size_t)q + 2u];
        B best;
        best.start(q, args);
        if (finite3(px, py, pz)) {
            best.search(r2);
            const float R = fmaxf(r * 1.0001f, 2.0e-18f);
            const int qx = (int)cell_coord(px, g.lox, g.cell, g.nx), qy = (int)cell_coord(py, g.loy, g.cell, g.ny), qz = (int)cell_coord(pz, g.loz, g.cell, g.nz);
            const int x0 = (int)cell_coord(px - R, g.lox, g.cell, g.nx), x1 = (int)cell_coord(px + R, g.lox, g.cell, g.nx);
            const int y0 = (int)cell_coord(py - R, g.loy, g.cell, g.ny), y1 = (int)cell_coord(py + R, g.loy, g.cell, g.ny);
            const int z0 = (int)cell_coord(pz - R, g.loz, g.cell, g.nz), z1 = (int)cell_coord(pz + R, g.loz, g.cell, g.nz);
            const int kmax = max(max(max(qx - x0, x1 - qx), max(qy - y0, y1 - qy)), max(qz - z0, z1 - qz));
            for (int k = 0; k <= kmax; k++) {
                const int xa = max(x0, qx - k), xb = min(x1, qx + k);
                for (int z = max(z0, qz - k); z <= min(z1, qz + k); z++) {
                    const bool zface = (z == qz - k) || (z == qz + k);
                    for (int y = max(y0, qy - k); y <= min(y1, qy + k); y++) {
                        const u32 row = ((u32)z * g.ny + (u32)y) * g.nx;
                        if (zface || y == qy - k || y == qy + k) {   // a whole run of the ring's cells along x: consecutive records
                            const u32 first = starts[row + (u32)xa], last = starts[row + (u32)xb + 1u];
                            if (COUNT) examined += last - first;
                            scan_records(records, first, last, px, py, pz, best);
                        } else {                                     // (k > 0) the ring's two end cells of this row
                            if (qx - k >= x0) {
                                const u32 first = starts[row + (u32)(qx - k)], last = starts[row + (u32)(qx - k) + 1u];
                                if (COUNT) examined += last - first;
                                scan_records(records, first, last, px, py, pz, best);
                            }
                            if (qx + k <= x1) {
                                const u32 first = starts[row + (u32)(qx + k)], last = starts[row + (u32)(qx + k) + 1u];
                                if (COUNT) examined += last - first;
                                scan_records(records, first, last, px, py, pz, best);
                            }
                        }
                    }
                }
                const float T = ((float)k * g.cell - g.slack) * 0.9999f;
                if (T > 0.0f && best.worst() < T * T) break;
            }
            best.finish();
        }
        best.write(q, d2_out, index_out);
    }
    if (COUNT) {
#pragma unroll
        for (u32 d = 32; d >= 1; d >>= 1) examined += (unsigned long long)__shfl_xor((long long)examined, (int)d, 64);
        if ((threadIdx.x & 63u) == 0u && examined) atomicAdd(pairs, examined);
    }
}

__global__ __launch_bounds__(256) void fill_nothing_found_kernel(u32 K, float* __restrict__ d2_out, u32* __restrict__ index_out) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= K) return;
    d2_out[i] = __builtin_inff();
    index_out[i] = NO_INDEX;
}

// ---------------------------------------------------------------- 3. distance statistics
// out: u64 { n_found, n_within, sum_q }: the finite d2, those <= t2, and the sum of u32((sqrt(d2) / max_distance) 2^24) over the found; integer atomics
__global__ __launch_bounds__(256) void distance_stats_kernel(const float* __restrict__ d2, u32 K, float max_distance, float t2, unsigned long long* __restrict__ out) {
    __shared__ unsigned long long s_w[3][4];
    unsigned long long found = 0ull, within = 0ull, sum_q = 0ull;
    for (u32 i = blockIdx.x * 256u + threadIdx.x; i < K; i += gridDim.x * 256u) {
        const float v = d2[i];
        if (fabsf(v) < __builtin_inff()) {
            found += 1ull;
            sum_q += (unsigned long long)wd_to_u32(wd_div(wd_sqrt(v), max_distance) * 16777216.0f);
        }
        if (v <= t2) within += 1ull;
    }
#pragma unroll
    for (u32 d = 32; d >= 1; d >>= 1) {
        found += (unsigned long long)__shfl_xor((long long)found, (int)d, 64);
        within += (unsigned long long)__shfl_xor((long long)within, (int)d, 64);
        sum_q += (unsigned long long)__shfl_xor((long long)sum_q, (int)d, 64);
    }
    if ((threadIdx.x & 63u) == 0u) { s_w[0][threadIdx.x >> 6] = found; s_w[1][threadIdx.x >> 6] = within; s_w[2][threadIdx.x >> 6] = sum_q; }
    __syncthreads();
    if (threadIdx.x < 3u) {
        const unsigned long long s = s_w[threadIdx.x][0] + s_w[threadIdx.x][1] + s_w[threadIdx.x][2] + s_w[threadIdx.x][3];
        if (s) atomicAdd(out + threadIdx.x, s);
    }
}

// ---------------------------------------------------------------- 4. scales from the neighbours (section 15)
// positions[i] = halves 0, 1, 2 of record i (u32[6]: position and opacity, rotation, log scale and one spare half) as f32: what the renderer sees
__global__ __launch_bounds__(256) void unpack_positions_kernel(const u32* __restrict__ gaussians, u32 N, float* __restrict__ positions) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= N) return;
    const u32 w0 = gaussians[6u * (size_t)i], w1 = gaussians[6u * (size_t)i + 1u];
    positions[3u * (size_t)i] = wd_unpack_lo(w0);
    positions[3u * (size_t)i + 1u] = wd_unpack_hi(w0);
    positions[3u * (size_t)i + 2u] = wd_unpack_lo(w1);
}

// One thread per point: the mean of the finite slots of its row of d2 (summed from slot 0; the finite slots come first), clamped from below, and
// log sigma = 0.5 log(mean) as fp16 into halves 8, 9, 10 of its record.  A row without a finite slot leaves the record alone.
__global__ __launch_bounds__(256) void neighbour_scales_kernel(u32* __restrict__ gaussians, u32 N, const float* __restrict__ d2, u32 k, float min_d2,
                                                               float* __restrict__ mean_out) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= N) return;
    const float* row = d2 + (size_t)i * k;
    float s = 0.0f;
    u32 found = 0u;
    for (u32 j = 0; j < k; j++) {
        const float v = row[j];
        if (fabsf(v) < __builtin_inff()) {
            s = s + v;
            found++;
        }
    }
    float mean = __builtin_inff();
    if (found) {
        mean = wd_div(s, (float)found);
        const u32 h = wd_f16bits(0.5f * wd_log(fmaxf(mean, min_d2)));
        u32* w = gaussians + 6u * (size_t)i;
        w[4] = h | (h << 16);
        w[5] = (w[5] & 0xFFFF0000u) | h;
    }
    if (mean_out) mean_out[i] = mean;
}

bool positive_finite(float x) { return x > 0.0f && x < __builtin_inff(); }

}  // namespace

// ---------------------------------------------------------------- launchers
int launch_sample_count(wdgs_device* dev, const float* vertices, u32 V, const u32* faces, u32 F, float density, u32 seed, u32* counts, unsigned long long* total) {
    WDGS_CHECK_HIP(hipMemsetAsync(total, 0, 8, dev->stream));
    if (F == 0) return WDGS_OK;
    WDGS_LAUNCH(dev, "sample_count", sample_count_kernel, dim3(ceil_div(F, 256u)), dim3(256), 0, vertices, V, faces, F, density, seed, counts, total);
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

int launch_sample_emit(wdgs_device* dev, const float* vertices, u32 V, const u32* faces, u32 F, u32 seed, const u32* offsets, u32 total, float* points, u32* face_out) {
    if (total == 0 || F == 0) return WDGS_OK;
    WDGS_LAUNCH(dev, "sample_emit", sample_emit_kernel, dim3(ceil_div(total, 256u)), dim3(256), 0, vertices, V, faces, F, seed, offsets, total, points, face_out);
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

int launch_point_bounds(wdgs_device* dev, const float* points, u32 M, u32* bounds7) {
    WDGS_CHECK_HIP(hipMemsetAsync(bounds7, 0xFF, 12, dev->stream));
    WDGS_CHECK_HIP(hipMemsetAsync(bounds7 + 3, 0, 16, dev->stream));
    if (M == 0) return WDGS_OK;
    const u32 grid = std::min<u32>(ceil_div(M, 256u), (u32)dev->num_cus * 4u);
    WDGS_LAUNCH(dev, "point_bounds", point_bounds_kernel, dim3(grid), dim3(256), 0, points, M, bounds7);
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

int launch_point_distance_stats(wdgs_device* dev, const float* d2, u32 K, float max_distance, float threshold, unsigned long long* out3) {
    WDGS_CHECK_HIP(hipMemsetAsync(out3, 0, 24, dev->stream));
    if (K == 0) return WDGS_OK;
    const u32 grid = std::min<u32>(ceil_div(K, 256u), (u32)dev->num_cus * 4u);
    WDGS_LAUNCH(dev, "distance_stats", distance_stats_kernel, dim3(grid), dim3(256), 0, d2, K, max_distance, threshold * threshold, out3);
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

// ---------------------------------------------------------------- the C ABI objects (include/webdgs.h)
struct wdgs_mesh_sampler {
    wdgs_device* dev = nullptr;
    DevMem<u32> counts, offsets;   // per triangle: the sample count and its exclusive scan
    DevMem<u32> scan_total;        // the scan's own (u32) total: unused, the u64 sum decides
    DevMem<unsigned long long> total;
    ScanScratch scan;
    u32 capacity = 0;              // triangles the buffers hold
    // emit is valid only for the arguments the last successful count saw
    bool counted = false;
    const void* vertices = nullptr;
    const void* faces = nullptr;
    u32 V = 0, F = 0, seed = 0, counted_total = 0;
    float density = 0.f;
};

extern "C" int wdgs_mesh_sampler_create(wdgs_device* dev, wdgs_mesh_sampler** out) {
    WDGS_REQUIRE(dev && out, WDGS_E_INVALID, "wdgs_mesh_sampler_create: null argument");
    WDGS_REQUIRE(!dev->capturing, WDGS_E_STATE, "wdgs_mesh_sampler_create while recording a command buffer");
    auto s = std::make_unique<wdgs_mesh_sampler>();
    s->dev = dev;
    WDGS_TRY(s->total.alloc(1, true, dev->stream));
    WDGS_TRY(s->scan_total.alloc(1, true, dev->stream));
    *out = s.release();
    return WDGS_OK;
}

extern "C" int wdgs_mesh_sampler_destroy(wdgs_mesh_sampler* s) {
    if (!s) return WDGS_OK;
    if (wdgs_device_alive(s->dev) && !s->dev->capturing) (void)wdgs_sync_lanes(s->dev);
    delete s;
    return WDGS_OK;
}

extern "C" int wdgs_mesh_sampler_count(wdgs_mesh_sampler* s, const void* vertices_f32_dev, uint32_t num_vertices, const void* faces_u32_dev, uint32_t num_faces, float density,
                                       uint32_t seed, uint64_t* total) {
    WDGS_REQUIRE(s && total, WDGS_E_INVALID, "wdgs_mesh_sampler_count: null argument");
    WDGS_REQUIRE(num_faces == 0 || (vertices_f32_dev && faces_u32_dev), WDGS_E_INVALID, "wdgs_mesh_sampler_count: null mesh");
    WDGS_REQUIRE(positive_finite(density), WDGS_E_INVALID, "wdgs_mesh_sampler_count: the density must be positive and finite (got %g)", (double)density);
    WDGS_REQUIRE((((uintptr_t)vertices_f32_dev | (uintptr_t)faces_u32_dev) & 3u) == 0u, WDGS_E_INVALID, "wdgs_mesh_sampler_count: misaligned mesh");
    wdgs_device* d = s->dev;
    WDGS_REQUIRE(!d->capturing, WDGS_E_STATE, "sampleMesh: the count waits for its total and cannot be recorded into a command buffer");
    s->counted = false;
    *total = 0;
    if (num_faces > s->capacity) {
        WDGS_CHECK_HIP(wdgs_sync_lanes(d));   // (nothing in flight may still read the blocks given back)
        s->capacity = 0;
        WDGS_TRY(s->counts.alloc(num_faces, false, d->stream));
        WDGS_TRY(s->offsets.alloc(num_faces, false, d->stream));
        WDGS_TRY(scan_scratch_create(&s->scan, num_faces));
        s->capacity = num_faces;
    }
    WDGS_TRY(launch_sample_count(d, static_cast<const float*>(vertices_f32_dev), num_vertices, static_cast<const u32*>(faces_u32_dev), num_faces, density, seed, s->counts,
                                 s->total));
    unsigned long long n = 0;
    WDGS_CHECK_HIP(hipMemcpyAsync(&n, s->total, sizeof(n), hipMemcpyDeviceToHost, d->stream));
    WDGS_CHECK_HIP(wdgs_sync_lanes(d));
    *total = n;
    // (counts saturate at 2^31 - 1 each and the scan is u32: below 2^31 in all, no offset can wrap)
    WDGS_REQUIRE(n < (1ull << 31), WDGS_E_CAPACITY, "sampleMesh: %llu samples, 2^31 or more (lower the density)", n);
    WDGS_TRY(scan_exclusive_u32(d, &s->scan, s->counts, s->offsets, num_faces, s->scan_total));
    s->vertices = vertices_f32_dev;
    s->faces = faces_u32_dev;
    s->V = num_vertices;
    s->F = num_faces;
    s->density = density;
    s->seed = seed;
    s->counted_total = (u32)n;
    s->counted = true;
    return WDGS_OK;
}

extern "C" int wdgs_mesh_sampler_emit(wdgs_mesh_sampler* s, const void* vertices_f32_dev, uint32_t num_vertices, const void* faces_u32_dev, uint32_t num_faces, float density,
                                      uint32_t seed, void* points_f32_dev, void* face_u32_dev, uint32_t capacity_samples) {
    WDGS_REQUIRE(s, WDGS_E_INVALID, "wdgs_mesh_sampler_emit: null sampler");
    WDGS_REQUIRE(s->counted, WDGS_E_STATE, "sampleMesh: no count precedes the emit");
    WDGS_REQUIRE(s->vertices == vertices_f32_dev && s->faces == faces_u32_dev && s->V == num_vertices && s->F == num_faces && s->seed == seed &&
                     memcmp(&s->density, &density, sizeof(float)) == 0,
                 WDGS_E_STATE, "sampleMesh: the emit's arguments are not those of the count before it (count again)");
    WDGS_REQUIRE(capacity_samples >= s->counted_total, WDGS_E_CAPACITY, "sampleMesh: %u samples, room for %u", s->counted_total, capacity_samples);
    if (s->counted_total == 0) return WDGS_OK;
    WDGS_REQUIRE(points_f32_dev, WDGS_E_INVALID, "wdgs_mesh_sampler_emit: null points");
    WDGS_REQUIRE((((uintptr_t)points_f32_dev | (uintptr_t)face_u32_dev) & 3u) == 0u, WDGS_E_INVALID, "wdgs_mesh_sampler_emit: misaligned output");
    return launch_sample_emit(s->dev, static_cast<const float*>(vertices_f32_dev), num_vertices, static_cast<const u32*>(faces_u32_dev), num_faces, seed, s->offsets,
                              s->counted_total, static_cast<float*>(points_f32_dev), static_cast<u32*>(face_u32_dev));
}

struct wdgs_point_index {
    wdgs_device* dev = nullptr;
    const float* points = nullptr;   // the caller's, read by the build only
    u32 M = 0, indexed = 0;          // points given, finite points kept
    float lo[3] = {0.f, 0.f, 0.f}, hi[3] = {0.f, 0.f, 0.f};
    double extent[3] = {0., 0., 0.};
    bool built = false;
    PointGrid g = {0.f, 0.f, 0.f, 1.f, 1u, 1u, 1u, 0.f};
    u32 cells = 1;
    DevMem<u32> bounds;              // point_bounds_kernel's seven words
    DevMem<float4> records;          // the cell-sorted copy
    DevMem<u32> counts, starts;      // per cell; starts has cells + 1 entries.  counts serves the queries after the build
    DevMem<u32> query_starts;        // per cell: where a cell's queries begin in `order`
    DevMem<u32> cell_of, rank, order;   // per point during the build, per query afterwards
    u32 query_capacity = 0;
    ScanScratch scan;
    DevMem<u32> scan_total;
};

// The grid for a cell edge: the edge is enlarged until the cells number 2^26 at most; count -> scan -> scatter.  Eager only (it allocates).
static int point_index_build_grid(wdgs_point_index* ix, float cell) {
    wdgs_device* d = ix->dev;
    double c = (double)cell;
    uint64_t n[3];
    for (;;) {
        bool fits = std::isfinite(c);
        uint64_t total = 1;
        for (int a = 0; a < 3 && fits; a++) {
            const double q = std::floor(ix->extent[a] / c) + 1.0;
            fits = q <= (double)MAX_CELLS;
            n[a] = fits ? (uint64_t)q : 0;
            if (fits) { total *= n[a]; fits = total <= MAX_CELLS; }
        }
        if (fits) break;
        if (!std::isfinite(c)) { n[0] = n[1] = n[2] = 1; c = (double)cell; break; }   // (an extent beyond every finite edge: one cell)
        c *= 1.25;
    }
    float cf = (float)c;
    if (!(cf < __builtin_inff())) { cf = 3.0e38f; n[0] = n[1] = n[2] = 1; }
    const double widest = std::max(ix->extent[0], std::max(ix->extent[1], ix->extent[2]));
    // cell_coord's quotient is off by at most 2^-22 of its value, i.e. 2^-22 of the extent in world units, on either side of a pair: 2^-20 covers it twice over
    const float slack = std::nextafter((float)(widest * 9.5367431640625e-07), __builtin_inff());
    ix->g = PointGrid{ix->lo[0], ix->lo[1], ix->lo[2], cf, (u32)n[0], (u32)n[1], (u32)n[2], slack};
    ix->cells = (u32)(n[0] * n[1] * n[2]);
    WDGS_TRY(ix->counts.alloc(ix->cells, true, d->stream));
    WDGS_TRY(ix->starts.alloc((size_t)ix->cells + 1u, true, d->stream));
    WDGS_TRY(ix->query_starts.alloc(ix->cells, false, d->stream));
    WDGS_TRY(ix->records.alloc(std::max<u32>(ix->indexed, 1u), false, d->stream));
    WDGS_TRY(scan_scratch_create(&ix->scan, ix->cells));
    if (ix->M) {
        WDGS_LAUNCH(d, "point_cell", point_cell_kernel, dim3(ceil_div(ix->M, 256u)), dim3(256), 0, ix->g, ix->points, ix->M, 0u, ix->cell_of, ix->rank, ix->counts);
        WDGS_CHECK_HIP(hipGetLastError());
        WDGS_TRY(scan_exclusive_u32(d, &ix->scan, ix->counts, ix->starts, ix->cells, ix->starts + ix->cells));
        WDGS_LAUNCH(d, "point_scatter", point_scatter_kernel, dim3(ceil_div(ix->M, 256u)), dim3(256), 0, ix->points, ix->M, ix->cell_of, ix->rank, ix->starts, ix->records);
        WDGS_CHECK_HIP(hipGetLastError());
    }
    ix->built = true;
    return WDGS_OK;
}

static int point_index_reserve(wdgs_point_index* ix, u32 K) {
    if (K <= ix->query_capacity) return WDGS_OK;
    wdgs_device* d = ix->dev;
    WDGS_REQUIRE(!d->capturing, WDGS_E_STATE, "PointIndex: %u queries exceed the %u reserved and a recording cannot allocate (reserveQueries, or one eager query of that size, first)", K,
                 ix->query_capacity);
    WDGS_CHECK_HIP(wdgs_sync_lanes(d));   // (nothing in flight may still read the blocks given back)
    ix->query_capacity = 0;
    WDGS_TRY(ix->cell_of.alloc(K, false, d->stream));
    WDGS_TRY(ix->rank.alloc(K, false, d->stream));
    WDGS_TRY(ix->order.alloc(K, false, d->stream));
    ix->query_capacity = K;
    return WDGS_OK;
}

extern "C" int wdgs_point_index_create(wdgs_device* dev, const void* points_f32_dev, uint64_t num_points, float cell_size, wdgs_point_index** out) {
    WDGS_REQUIRE(dev && out, WDGS_E_INVALID, "wdgs_point_index_create: null argument");
    WDGS_REQUIRE(num_points <= 0x7FFFFFFFull, WDGS_E_INVALID, "wdgs_point_index_create: %llu points, more than 2^31 - 1", (unsigned long long)num_points);
    WDGS_REQUIRE(num_points == 0 || points_f32_dev, WDGS_E_INVALID, "wdgs_point_index_create: null points");
    WDGS_REQUIRE(((uintptr_t)points_f32_dev & 3u) == 0u, WDGS_E_INVALID, "wdgs_point_index_create: misaligned points");
    WDGS_REQUIRE(cell_size == 0.0f || positive_finite(cell_size), WDGS_E_INVALID, "wdgs_point_index_create: the cell edge must be positive and finite, or 0 (got %g)",
                 (double)cell_size);
    WDGS_REQUIRE(!dev->capturing, WDGS_E_STATE, "PointIndex: the build reads its bounds back and cannot be recorded into a command buffer");
    auto ix = std::make_unique<wdgs_point_index>();
    ix->dev = dev;
    ix->points = static_cast<const float*>(points_f32_dev);
    ix->M = (u32)num_points;
    WDGS_TRY(ix->bounds.alloc(8, true, dev->stream));
    WDGS_TRY(ix->scan_total.alloc(1, true, dev->stream));
    WDGS_TRY(point_index_reserve(ix.get(), std::max<u32>(ix->M, 1u)));
    WDGS_TRY(launch_point_bounds(dev, ix->points, ix->M, ix->bounds));
    u32 b[7] = {0, 0, 0, 0, 0, 0, 0};
    WDGS_CHECK_HIP(hipMemcpyAsync(b, ix->bounds, sizeof(b), hipMemcpyDeviceToHost, dev->stream));
    WDGS_CHECK_HIP(wdgs_sync_lanes(dev));
    ix->indexed = b[6];
    if (ix->indexed) {
        for (int a = 0; a < 3; a++) {
            ix->lo[a] = from_ordered_bits(b[a]);
            ix->hi[a] = from_ordered_bits(b[3 + a]);
            ix->extent[a] = (double)ix->hi[a] - (double)ix->lo[a];
        }
    }
    if (cell_size != 0.0f) WDGS_TRY(point_index_build_grid(ix.get(), cell_size));
    *out = ix.release();
    return WDGS_OK;
}

extern "C" int wdgs_point_index_destroy(wdgs_point_index* ix) {
    if (!ix) return WDGS_OK;
    if (wdgs_device_alive(ix->dev) && !ix->dev->capturing) (void)wdgs_sync_lanes(ix->dev);
    delete ix;
    return WDGS_OK;
}

extern "C" int wdgs_point_index_reserve_queries(wdgs_point_index* ix, uint32_t num_queries) {
    WDGS_REQUIRE(ix, WDGS_E_INVALID, "wdgs_point_index_reserve_queries: null index");
    WDGS_REQUIRE(num_queries <= 0x7FFFFFFFu, WDGS_E_INVALID, "wdgs_point_index_reserve_queries: %u queries, more than 2^31 - 1", num_queries);
    return point_index_reserve(ix, num_queries);
}

extern "C" int wdgs_point_index_info(const wdgs_point_index* ix, float* cell_size, uint32_t* dims3, uint32_t* indexed_points) {
    WDGS_REQUIRE(ix, WDGS_E_INVALID, "wdgs_point_index_info: null index");
    if (cell_size) *cell_size = ix->built ? ix->g.cell : 0.0f;
    if (dims3) { dims3[0] = ix->built ? ix->g.nx : 0u; dims3[1] = ix->built ? ix->g.ny : 0u; dims3[2] = ix->built ? ix->g.nz : 0u; }
    if (indexed_points) *indexed_points = ix->indexed;
    return WDGS_OK;
}

extern "C" int wdgs_point_index_bounds(const wdgs_point_index* ix, float* lo3, float* hi3) {
    WDGS_REQUIRE(ix, WDGS_E_INVALID, "wdgs_point_index_bounds: null index");
    for (int a = 0; a < 3; a++) {
        if (lo3) lo3[a] = ix->lo[a];
        if (hi3) hi3[a] = ix->hi[a];
    }
    return WDGS_OK;
}

// What both queries do before their kernel: the grid of an index created with a cell edge of 0 (the first query's cutoff, or the edge at which a cube of
// the widest extent holds one cell per point if smaller), and the queries bucketed by cell into ix->order.  Not called for K = 0 or an empty index.
static int point_index_ensure_grid(wdgs_point_index* ix, float max_distance, const char* who) {
    if (ix->built) return WDGS_OK;
    WDGS_REQUIRE(!ix->dev->capturing, WDGS_E_STATE, "PointIndex.%s: the index has no grid yet (cell edge 0) and its first query, which builds it, cannot be recorded", who);
    float edge = max_distance;
    const double widest = std::max(ix->extent[0], std::max(ix->extent[1], ix->extent[2]));
    if (ix->indexed && std::isfinite(widest)) {
        const float by_count = (float)(widest / std::cbrt((double)ix->indexed));
        if (positive_finite(by_count) && by_count < edge) edge = by_count;
    }
    return point_index_build_grid(ix, edge);
}

static int point_index_order_queries(wdgs_point_index* ix, const float* queries, u32 K) {
    wdgs_device* d = ix->dev;
    const u32 blocks = ceil_div(K, 256u);
    WDGS_TRY(point_index_reserve(ix, K));
    WDGS_CHECK_HIP(hipMemsetAsync(ix->counts, 0, (size_t)ix->cells * sizeof(u32), d->stream));
    WDGS_LAUNCH(d, "query_cell", point_cell_kernel, dim3(blocks), dim3(256), 0, ix->g, queries, K, 1u, ix->cell_of, ix->rank, ix->counts);
    WDGS_CHECK_HIP(hipGetLastError());
    WDGS_TRY(scan_exclusive_u32(d, &ix->scan, ix->counts, ix->query_starts, ix->cells, ix->scan_total));
    WDGS_LAUNCH(d, "query_order", query_order_kernel, dim3(blocks), dim3(256), 0, K, ix->cell_of, ix->rank, ix->query_starts, ix->order);
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

extern "C" int wdgs_point_index_nearest(wdgs_point_index* ix, const void* queries_f32_dev, uint32_t num_queries, float max_distance, void* d2_f32_dev, void* index_u32_dev,
                                        void* pairs_u64_dev) {
    WDGS_REQUIRE(ix, WDGS_E_INVALID, "wdgs_point_index_nearest: null index");
    WDGS_REQUIRE(positive_finite(max_distance), WDGS_E_INVALID, "PointIndex.nearest: max_distance must be positive and finite (got %g)", (double)max_distance);
    WDGS_REQUIRE(num_queries <= 0x7FFFFFFFu, WDGS_E_INVALID, "PointIndex.nearest: %u queries, more than 2^31 - 1", num_queries);
    WDGS_REQUIRE(num_queries == 0 || (queries_f32_dev && d2_f32_dev && index_u32_dev), WDGS_E_INVALID, "wdgs_point_index_nearest: null argument");
    WDGS_REQUIRE((((uintptr_t)queries_f32_dev | (uintptr_t)d2_f32_dev | (uintptr_t)index_u32_dev) & 3u) == 0u && ((uintptr_t)pairs_u64_dev & 7u) == 0u, WDGS_E_INVALID,
                 "wdgs_point_index_nearest: misaligned argument");
    wdgs_device* d = ix->dev;
    WDGS_TRY(point_index_ensure_grid(ix, max_distance, "nearest"));
    if (num_queries == 0) return WDGS_OK;
    const u32 K = num_queries, blocks = ceil_div(K, 256u);
    float* d2 = static_cast<float*>(d2_f32_dev);
    u32* index = static_cast<u32*>(index_u32_dev);
    if (ix->indexed == 0) {
        WDGS_LAUNCH(d, "nearest_fill", fill_nothing_found_kernel, dim3(blocks), dim3(256), 0, K, d2, index);
        WDGS_CHECK_HIP(hipGetLastError());
        return WDGS_OK;
    }
    const float* queries = static_cast<const float*>(queries_f32_dev);
    WDGS_TRY(point_index_order_queries(ix, queries, K));
    const float r2 = max_distance * max_distance;
    unsigned long long* pairs = static_cast<unsigned long long*>(pairs_u64_dev);
    const auto kernel = pairs ? nearest_kernel<Best, true> : nearest_kernel<Best, false>;
    WDGS_LAUNCH(d, "nearest", kernel, dim3(blocks), dim3(256), 0, ix->g, ix->records, ix->starts, queries, ix->order, K, max_distance, r2, d2, index, pairs, Best::Args{});
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

template <u32 CAP>
static int launch_k_nearest(wdgs_point_index* ix, const float* queries, u32 K, u32 k, u32 exclude_self, float r, float* d2, u32* index, unsigned long long* pairs) {
    wdgs_device* d = ix->dev;
    const float r2 = r * r;
    const auto kernel = pairs ? nearest_kernel<BestK<CAP>, true> : nearest_kernel<BestK<CAP>, false>;
    WDGS_LAUNCH(d, "k_nearest", kernel, dim3(ceil_div(K, 256u)), dim3(256), 0, ix->g, ix->records, ix->starts, queries, ix->order, K, r, r2, d2, index, pairs,
                (typename BestK<CAP>::Args{k, exclude_self}));
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

extern "C" int wdgs_point_index_k_nearest(wdgs_point_index* ix, const void* queries_f32_dev, uint32_t num_queries, uint32_t k, float max_distance, uint32_t flags,
                                          void* d2_f32_dev, void* index_u32_dev, void* pairs_u64_dev) {
    WDGS_REQUIRE(ix, WDGS_E_INVALID, "wdgs_point_index_k_nearest: null index");
    WDGS_REQUIRE(k >= 1u && k <= WDGS_KNN_MAX_K, WDGS_E_INVALID, "PointIndex.kNearest: k must lie in [1, %u] (got %u)", (unsigned)WDGS_KNN_MAX_K, k);
    WDGS_REQUIRE((flags & ~(uint32_t)WDGS_KNN_EXCLUDE_SELF) == 0u, WDGS_E_INVALID, "PointIndex.kNearest: unknown flag bits 0x%x", flags);
    WDGS_REQUIRE(positive_finite(max_distance), WDGS_E_INVALID, "PointIndex.kNearest: max_distance must be positive and finite (got %g)", (double)max_distance);
    WDGS_REQUIRE(num_queries <= 0x7FFFFFFFu, WDGS_E_INVALID, "PointIndex.kNearest: %u queries, more than 2^31 - 1", num_queries);
    WDGS_REQUIRE((uint64_t)num_queries * k <= 0xFFFFFFFFull, WDGS_E_INVALID, "PointIndex.kNearest: %u queries times k = %u, more than 2^32 - 1 slots", num_queries, k);
    WDGS_REQUIRE(num_queries == 0 || (queries_f32_dev && d2_f32_dev && index_u32_dev), WDGS_E_INVALID, "wdgs_point_index_k_nearest: null argument");
    WDGS_REQUIRE((((uintptr_t)queries_f32_dev | (uintptr_t)d2_f32_dev | (uintptr_t)index_u32_dev) & 3u) == 0u && ((uintptr_t)pairs_u64_dev & 7u) == 0u, WDGS_E_INVALID,
                 "wdgs_point_index_k_nearest: misaligned argument");
    wdgs_device* d = ix->dev;
    WDGS_TRY(point_index_ensure_grid(ix, max_distance, "kNearest"));
    if (num_queries == 0) return WDGS_OK;
    const u32 K = num_queries;
    float* d2 = static_cast<float*>(d2_f32_dev);
    u32* index = static_cast<u32*>(index_u32_dev);
    if (ix->indexed == 0) {
        WDGS_LAUNCH(d, "nearest_fill", fill_nothing_found_kernel, dim3(ceil_div(K * k, 256u)), dim3(256), 0, K * k, d2, index);
        WDGS_CHECK_HIP(hipGetLastError());
        return WDGS_OK;
    }
    const float* queries = static_cast<const float*>(queries_f32_dev);
    WDGS_TRY(point_index_order_queries(ix, queries, K));
    const u32 exclude_self = flags & WDGS_KNN_EXCLUDE_SELF;
    unsigned long long* pairs = static_cast<unsigned long long*>(pairs_u64_dev);
    if (k <= 4u) return launch_k_nearest<4>(ix, queries, K, k, exclude_self, max_distance, d2, index, pairs);
    if (k <= 8u) return launch_k_nearest<8>(ix, queries, K, k, exclude_self, max_distance, d2, index, pairs);
    return launch_k_nearest<16>(ix, queries, K, k, exclude_self, max_distance, d2, index, pairs);
}

extern "C" int wdgs_point_cloud_positions(wdgs_device* dev, const void* gaussians_dev, uint32_t num_points, void* positions_f32_dev) {
    WDGS_REQUIRE(dev && (num_points == 0 || (gaussians_dev && positions_f32_dev)), WDGS_E_INVALID, "wdgs_point_cloud_positions: null argument");
    WDGS_REQUIRE((((uintptr_t)gaussians_dev | (uintptr_t)positions_f32_dev) & 3u) == 0u, WDGS_E_INVALID, "wdgs_point_cloud_positions: misaligned argument");
    if (num_points == 0) return WDGS_OK;
    WDGS_LAUNCH(dev, "unpack_positions", unpack_positions_kernel, dim3(ceil_div(num_points, 256u)), dim3(256), 0, static_cast<const u32*>(gaussians_dev), num_points,
                static_cast<float*>(positions_f32_dev));
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

extern "C" int wdgs_point_cloud_neighbour_scales(wdgs_device* dev, void* gaussians_dev, uint32_t num_points, const void* d2_f32_dev, uint32_t k, float min_d2,
                                                 void* mean_d2_f32_dev) {
    WDGS_REQUIRE(dev && (num_points == 0 || (gaussians_dev && d2_f32_dev)), WDGS_E_INVALID, "wdgs_point_cloud_neighbour_scales: null argument");
    WDGS_REQUIRE(k >= 1u && k <= WDGS_KNN_MAX_K, WDGS_E_INVALID, "initScalesFromNeighbours: k must lie in [1, %u] (got %u)", (unsigned)WDGS_KNN_MAX_K, k);
    WDGS_REQUIRE(positive_finite(min_d2), WDGS_E_INVALID, "initScalesFromNeighbours: min_d2 must be positive and finite (got %g)", (double)min_d2);
    WDGS_REQUIRE((((uintptr_t)gaussians_dev | (uintptr_t)d2_f32_dev | (uintptr_t)mean_d2_f32_dev) & 3u) == 0u, WDGS_E_INVALID,
                 "wdgs_point_cloud_neighbour_scales: misaligned argument");
    if (num_points == 0) return WDGS_OK;
    WDGS_LAUNCH(dev, "neighbour_scales", neighbour_scales_kernel, dim3(ceil_div(num_points, 256u)), dim3(256), 0, static_cast<u32*>(gaussians_dev), num_points,
                static_cast<const float*>(d2_f32_dev), k, min_d2, static_cast<float*>(mean_d2_f32_dev));
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

extern "C" int wdgs_point_distance_stats(wdgs_device* dev, const void* d2_f32_dev, uint32_t count, float max_distance, float threshold, void* out_u64x3_dev) {
    WDGS_REQUIRE(dev && out_u64x3_dev && (count == 0 || d2_f32_dev), WDGS_E_INVALID, "wdgs_point_distance_stats: null argument");
    WDGS_REQUIRE(positive_finite(max_distance), WDGS_E_INVALID, "pointDistanceStats: max_distance must be positive and finite (got %g)", (double)max_distance);
    WDGS_REQUIRE(threshold > 0.0f && threshold <= max_distance, WDGS_E_INVALID, "pointDistanceStats: the threshold must lie in (0, max_distance] (got %g, max_distance %g)",
                 (double)threshold, (double)max_distance);
    WDGS_REQUIRE(((uintptr_t)d2_f32_dev & 3u) == 0u && ((uintptr_t)out_u64x3_dev & 7u) == 0u, WDGS_E_INVALID, "wdgs_point_distance_stats: misaligned argument");
    return launch_point_distance_stats(dev, static_cast<const float*>(d2_f32_dev), count, max_distance, threshold, static_cast<unsigned long long*>(out_u64x3_dev));
}
