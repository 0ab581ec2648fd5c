// Mesh adjacency, Taubin smoothing and area-weighted vertex normals on the device (no counterpart in the reference, which renders
// colour only).
//
// Every valid face owns six directed half-edge keys from * 2^32 | to: its three edges forward and backward.  One stable u64 sort of the 6 F slots (KeySort,
// keysort.hip) puts equal keys together in ascending slot order.  The distinct keys, ascending, ARE the neighbour lists: the low words of a vertex's run are
// its neighbours, ascending and without repeats.  The length of a run of equal keys is the number of valid faces on that edge: 1 is a boundary edge, 3 or more
// a non-manifold one -- and the head flags of a pair and of the two behind it tell 1, 2 and "3 or more" apart without any run length being stored.  The sorted
// slots themselves, unmerged, are what the normals walk: the forward slots of a vertex's run name each incident face once, in an order the sort fixes.
//
// A smoothing step is one thread per vertex that walks its row and sums its neighbours' positions in ascending neighbour order, in f32: the order of the sum
// is part of the definition (include/webdgs.h), so a row is summed by one lane and nothing is ever added atomically.  The normals alike.
//
// Section 16's to 18's rule holds: no spin-wait, no inter-workgroup flag, no look-back, no grid barrier, no float atomics; visibility comes from launch
// boundaries only.  There is no global atomic at all: every count leaves the workgroup as a row of partial sums that ma_fold adds in a later launch (one word
// that every wave adds to serialises in L2: it cost more than the sort).  ma_edges' boundary flags are racing stores of the one value 1 into words cleared
// by an earlier memset and read by later launches only.
#include <algorithm>
#include <cmath>
#include <memory>

#include "dmath.h"
#include "launch.h"

namespace {

typedef unsigned long long u64;

constexpr u32 MA_THREADS = 256;
constexpr u32 MA_WAVES = MA_THREADS / 64;
constexpr u64 MA_NO_KEY = ~0ull;
constexpr u32 MA_FACE_ROUNDS = 4;   // faces per thread of ma_half_edge_keys: its workgroup leaves one invalid count per 1024 faces
constexpr u32 MA_FACE_TILE = MA_THREADS * MA_FACE_ROUNDS;
constexpr u32 MA_PAIR_ROUNDS = 16;   // sorted pairs per thread of ma_edges: one row of two edge counts per 4096 pairs
constexpr u32 MA_PAIR_TILE = MA_THREADS * MA_PAIR_ROUNDS;
constexpr u32 MA_VERTEX_ROUNDS = 8;  // vertices per thread of ma_rows: one row of three vertex counts per 2048 vertices
constexpr u32 MA_VERTEX_TILE = MA_THREADS * MA_VERTEX_ROUNDS;
// The totals block, u32 words: the distinct keys (2^64 - 1 included when a face is invalid), then what ma_fold adds up: the invalid faces, ma_edges' and ma_rows' counts
constexpr u32 MA_T_DISTINCT = 0, MA_T_INVALID = 1, MA_T_BOUNDARY_EDGES = 2, MA_T_NON_MANIFOLD = 3, MA_T_BOUNDARY_VERTICES = 4, MA_T_ISOLATED = 5, MA_T_MAX_DEGREE = 6,
              MA_T_WORDS = 8;
// The per-vertex block rows[3][V], cleared before ma_edges: where the vertex's run of sorted slots begins and ends, and its boundary flag
constexpr u32 MA_R_FIRST = 0, MA_R_LAST = 1, MA_R_BOUNDARY = 2, MA_R_PLANES = 3;

__device__ __forceinline__ bool finite_bits(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }
__device__ __forceinline__ bool finite3(float x, float y, float z) { return finite_bits(x) && finite_bits(y) && finite_bits(z); }

// The sum of x over the wave, in every lane
__device__ __forceinline__ u32 wave_sum(u32 x) {
#pragma unroll
    for (u32 d = 32; d >= 1; d >>= 1) x += (u32)__shfl_xor((int)x, (int)d, 64);
    return x;
}
__device__ __forceinline__ u32 wave_max(u32 x) {
#pragma unroll
    for (u32 d = 32; d >= 1; d >>= 1) x = max(x, (u32)__shfl_xor((int)x, (int)d, 64));
    return x;
}

// The sum (or the maximum) of x over the workgroup, in thread 0; lds: one word per wave, free again after the call
template <bool MAX>
__device__ __forceinline__ u32 block_fold(u32 x, u32* lds) {
    x = MAX ? wave_max(x) : wave_sum(x);
    __syncthreads();
    if ((threadIdx.x & 63u) == 0u) lds[threadIdx.x >> 6] = x;
    __syncthreads();
    u32 n = 0u;
    if (threadIdx.x == 0u) {
#pragma unroll
        for (u32 w = 0; w < MA_WAVES; w++) n = MAX ? max(n, lds[w]) : n + lds[w];
    }
    return n;
}

// One thread per face, four faces in turn.  A valid face (three indices < V, pairwise different) writes keys[6 f + 2 j + d]: the edge from corner j to corner
// j + 1 forward (d = 0) and backward (d = 1).  An invalid face writes MA_NO_KEY six times; its indices are compared and never used.  partial[g]: the
// workgroup's invalid faces (a store; ma_fold adds the rows in a later launch).
__global__ __launch_bounds__(MA_THREADS) void ma_half_edge_keys_kernel(const u32* __restrict__ faces, u32 F, u32 V, u64* __restrict__ keys, u32* __restrict__ partial) {
    __shared__ u32 counts[MA_WAVES];
    u32 mine = 0u;
    for (u32 round = 0; round < MA_FACE_ROUNDS; round++) {
        const u64 f = (u64)blockIdx.x * MA_FACE_TILE + round * MA_THREADS + threadIdx.x;
        if (f >= (u64)F) break;
        u32 c[3];
#pragma unroll
        for (u32 j = 0; j < 3u; j++) c[j] = faces[3u * f + j];
        const bool valid = c[0] < V && c[1] < V && c[2] < V && c[0] != c[1] && c[1] != c[2] && c[0] != c[2];
        mine += valid ? 0u : 1u;
#pragma unroll
        for (u32 j = 0; j < 3u; j++) {
            const u32 a = c[j], b = c[(j + 1u) % 3u];
            keys[6u * f + 2u * j] = valid ? (((u64)a << 32) | b) : MA_NO_KEY;
            keys[6u * f + 2u * j + 1u] = valid ? (((u64)b << 32) | a) : MA_NO_KEY;
        }
    }
    const u32 n = block_fold<false>(mine, counts);
    if (threadIdx.x == 0u) partial[blockIdx.x] = n;
}

// One workgroup, after every other kernel of the count: adds the rows of partial counts into the totals block -- the faces' one word per row, the edges'
// two, the vertices' three, of which the last is a maximum
__global__ __launch_bounds__(MA_THREADS) void ma_fold_kernel(const u32* __restrict__ face_rows, u32 num_face_rows, const u32* __restrict__ edge_rows, u32 num_edge_rows,
                                                             const u32* __restrict__ vertex_rows, u32 num_vertex_rows, u32* __restrict__ totals) {
    __shared__ u32 lds[MA_WAVES];
    u32 invalid = 0u, boundary_edges = 0u, non_manifold = 0u, isolated = 0u, boundary_vertices = 0u, most = 0u;
    for (u32 g = threadIdx.x; g < num_face_rows; g += MA_THREADS) invalid += face_rows[g];
    for (u32 g = threadIdx.x; g < num_edge_rows; g += MA_THREADS) {
        boundary_edges += edge_rows[2u * g];
        non_manifold += edge_rows[2u * g + 1u];
    }
    for (u32 g = threadIdx.x; g < num_vertex_rows; g += MA_THREADS) {
        isolated += vertex_rows[3u * g];
        boundary_vertices += vertex_rows[3u * g + 1u];
        most = max(most, vertex_rows[3u * g + 2u]);
    }
    invalid = block_fold<false>(invalid, lds);
    boundary_edges = block_fold<false>(boundary_edges, lds);
    non_manifold = block_fold<false>(non_manifold, lds);
    isolated = block_fold<false>(isolated, lds);
    boundary_vertices = block_fold<false>(boundary_vertices, lds);
    most = block_fold<true>(most, lds);
    if (threadIdx.x != 0u) return;
    totals[MA_T_INVALID] = invalid;
    totals[MA_T_BOUNDARY_EDGES] = boundary_edges;
    totals[MA_T_NON_MANIFOLD] = non_manifold;
    totals[MA_T_ISOLATED] = isolated;
    totals[MA_T_BOUNDARY_VERTICES] = boundary_vertices;
    totals[MA_T_MAX_DEGREE] = most;
}

// One thread per sorted pair i, sixteen pairs in turn; flags, ids: the sort's head flags and their exclusive scan, so a head is distinct key number ids[i].  A
// pair of MA_NO_KEY does nothing: its high word is no vertex.  Every other key's words are < V.
//   a head:                     neighbours[ids[i]] = the key's low word; with no head behind it (a run of one) boundary[from] = 1 -- the reversed key's head
//                               flags the other end -- and with no head in the two pairs behind it the edge is non-manifold; edges are counted where from < to
//   the first pair of a vertex: rows[FIRST][from] = i          the last pair of a vertex: rows[LAST][from] = i + 1
// partial[2 g], partial[2 g + 1]: the workgroup's boundary and non-manifold edges
__global__ __launch_bounds__(MA_THREADS) void ma_edges_kernel(KeySortView b, u32 S, u32 V, const u32* __restrict__ flags, const u32* __restrict__ ids,
                                                              u32* __restrict__ neighbours, u32* __restrict__ rows, u32* __restrict__ partial) {
    __shared__ u32 lds[MA_WAVES];
    const u64* __restrict__ keys = b.sorted_keys();
    u32 boundary_edges = 0u, non_manifold = 0u;
    for (u32 round = 0; round < MA_PAIR_ROUNDS; round++) {
        const u64 i = (u64)blockIdx.x * MA_PAIR_TILE + round * MA_THREADS + threadIdx.x;
        if (i >= (u64)S) break;
        const u64 key = keys[i];
        if (key == MA_NO_KEY) continue;
        const u32 from = (u32)(key >> 32), to = (u32)key;
        const u64 next = i + 1ull < (u64)S ? keys[i + 1ull] : MA_NO_KEY;
        if (flags[i] != 0u) {
            neighbours[ids[i]] = to;
            const bool one = i + 1ull >= (u64)S || flags[i + 1ull] != 0u;
            const bool many = i + 2ull < (u64)S && flags[i + 1ull] == 0u && flags[i + 2ull] == 0u;
            if (one) rows[(size_t)MA_R_BOUNDARY * V + from] = 1u;
            if (from < to) {
                boundary_edges += one ? 1u : 0u;
                non_manifold += many ? 1u : 0u;
            }
        }
        if (i == 0ull || (u32)(keys[i - 1ull] >> 32) != from) rows[(size_t)MA_R_FIRST * V + from] = (u32)i;
        if (next == MA_NO_KEY || (u32)(next >> 32) != from) rows[(size_t)MA_R_LAST * V + from] = (u32)i + 1u;
    }
    boundary_edges = block_fold<false>(boundary_edges, lds);
    non_manifold = block_fold<false>(non_manifold, lds);
    if (threadIdx.x == 0u) {
        partial[2u * blockIdx.x] = boundary_edges;
        partial[2u * blockIdx.x + 1u] = non_manifold;
    }
}

// One thread per vertex, eight vertices in turn, and one more for degree[V] = 0 (so that the exclusive scan of degree[V + 1] ends in E).  A vertex's degree is
// the number of heads in its run of sorted pairs: the distinct-key number behind its last pair less that of its first.  An unused vertex has the cleared,
// empty run.  partial[3 g ..]: the workgroup's isolated vertices, its boundary vertices and its largest degree
__global__ __launch_bounds__(MA_THREADS) void ma_rows_kernel(u32 V, const u32* __restrict__ flags, const u32* __restrict__ ids, const u32* __restrict__ rows,
                                                             u32* __restrict__ degree, u32* __restrict__ partial) {
    __shared__ u32 lds[MA_WAVES];
    u32 isolated = 0u, on_boundary = 0u, most = 0u;
    for (u32 round = 0; round < MA_VERTEX_ROUNDS; round++) {
        const u64 v = (u64)blockIdx.x * MA_VERTEX_TILE + round * MA_THREADS + threadIdx.x;
        if (v > (u64)V) break;
        u32 deg = 0u;
        if (v < (u64)V) {
            const u32 first = rows[(size_t)MA_R_FIRST * V + v], last = rows[(size_t)MA_R_LAST * V + v];
            if (last > first) deg = ids[last - 1u] + flags[last - 1u] - ids[first];
            isolated += deg == 0u ? 1u : 0u;
            on_boundary += rows[(size_t)MA_R_BOUNDARY * V + v];
            most = max(most, deg);
        }
        degree[v] = deg;
    }
    isolated = block_fold<false>(isolated, lds);
    on_boundary = block_fold<false>(on_boundary, lds);
    most = block_fold<true>(most, lds);
    if (threadIdx.x == 0u) {
        partial[3u * blockIdx.x] = isolated;
        partial[3u * blockIdx.x + 1u] = on_boundary;
        partial[3u * blockIdx.x + 2u] = most;
    }
}

// The three outputs of emit, each nullable: row_start[V + 1], neighbours[E], boundary[V]
__global__ __launch_bounds__(MA_THREADS) void ma_emit_kernel(u32 V, u32 E, const u32* __restrict__ row_start, const u32* __restrict__ neighbours, const u32* __restrict__ boundary,
                                                             u32* __restrict__ row_start_out, u32* __restrict__ neighbours_out, u32* __restrict__ boundary_out) {
    const u32 i = blockIdx.x * MA_THREADS + threadIdx.x;
    if (row_start_out && i <= V) row_start_out[i] = row_start[i];
    if (neighbours_out && i < E) neighbours_out[i] = neighbours[i];
    if (boundary_out && i < V) boundary_out[i] = boundary[i];
}

__global__ __launch_bounds__(MA_THREADS) void ma_copy_kernel(const u32* __restrict__ in, u32* __restrict__ out, size_t words) {
    const size_t i = (size_t)blockIdx.x * MA_THREADS + threadIdx.x;
    if (i < words) out[i] = in[i];
}

// step(p, w) of include/webdgs.h, one thread per vertex: the row is walked by this lane alone, in ascending neighbour order.  in and out are different arrays.
__global__ __launch_bounds__(MA_THREADS) void ma_smooth_step_kernel(const float* __restrict__ in, float* __restrict__ out, u32 V, const u32* __restrict__ row_start,
                                                                    const u32* __restrict__ neighbours, const u32* __restrict__ boundary, u32 pin_boundary, float w) {
    const u32 v = blockIdx.x * MA_THREADS + threadIdx.x;
    if (v >= V) return;
    const float px = in[3u * (size_t)v], py = in[3u * (size_t)v + 1u], pz = in[3u * (size_t)v + 2u];
    float rx = px, ry = py, rz = pz;
    const bool pinned = pin_boundary != 0u && boundary[v] != 0u;
    if (!pinned && finite3(px, py, pz)) {
        float sx = 0.f, sy = 0.f, sz = 0.f;
        u32 n = 0u;
        const u32 end = row_start[v + 1u];
        for (u32 e = row_start[v]; e < end; e++) {
            const size_t u = neighbours[e];
            const float qx = in[3u * u], qy = in[3u * u + 1u], qz = in[3u * u + 2u];
            if (!finite3(qx, qy, qz)) continue;
            sx += qx; sy += qy; sz += qz;
            n++;
        }
        if (n != 0u) {
            const float fn = (float)n;
            const float mx = wd_div(sx, fn), my = wd_div(sy, fn), mz = wd_div(sz, fn);
            const float dx = mx - px, dy = my - py, dz = mz - pz;
            const float tx = w * dx, ty = w * dy, tz = w * dz;
            const float ox = px + tx, oy = py + ty, oz = pz + tz;
            if (finite3(ox, oy, oz)) { rx = ox; ry = oy; rz = oz; }
        }
    }
    out[3u * (size_t)v] = rx;
    out[3u * (size_t)v + 1u] = ry;
    out[3u * (size_t)v + 2u] = rz;
}

// One thread per vertex over its run of sorted pairs [rows[FIRST][v], rows[LAST][v]): ascending neighbour, then ascending slot.  A forward slot s = 6 f + 2 j
// (even) names the face f once for the corner it leaves; g_f is taken from the face's own corner order whichever corner asks.
__global__ __launch_bounds__(MA_THREADS) void ma_vertex_normals_kernel(const float* __restrict__ vertices, const u32* __restrict__ faces, u32 V, KeySortView b,
                                                                       const u32* __restrict__ rows, float* __restrict__ normals) {
    const u32 v = blockIdx.x * MA_THREADS + threadIdx.x;
    if (v >= V) return;
    const u32* __restrict__ slots = b.sorted_slots();
    const u32 first = rows[(size_t)MA_R_FIRST * V + v], last = rows[(size_t)MA_R_LAST * V + v];
    float sx = 0.f, sy = 0.f, sz = 0.f;
    u32 n = 0u;
    for (u32 i = first; i < last; i++) {
        const u32 slot = slots ? slots[i] : i;
        if ((slot & 1u) != 0u) continue;
        const size_t f = slot / 6u;
        const size_t c0 = faces[3u * f], c1 = faces[3u * f + 1u], c2 = faces[3u * f + 2u];
        if (c0 >= V || c1 >= V || c2 >= V) continue;   // (never with the counted faces: a face with a key is valid.  Faces changed since then address nothing)
        const float p0x = vertices[3u * c0], p0y = vertices[3u * c0 + 1u], p0z = vertices[3u * c0 + 2u];
        const float ax = vertices[3u * c1] - p0x, ay = vertices[3u * c1 + 1u] - p0y, az = vertices[3u * c1 + 2u] - p0z;
        const float bx = vertices[3u * c2] - p0x, by = vertices[3u * c2 + 1u] - p0y, bz = vertices[3u * c2 + 2u] - p0z;
        const float gx = ay * bz - az * by, gy = az * bx - ax * bz, gz = ax * by - ay * bx;
        if (!finite3(gx, gy, gz)) continue;
        sx += gx; sy += gy; sz += gz;
        n++;
    }
    const float q = (sx * sx + sy * sy) + sz * sz;
    float nx = 0.f, ny = 0.f, nz = 0.f;
    if (n != 0u && finite_bits(q) && q != 0.f) {
        const float len = wd_sqrt(q);
        nx = wd_div(sx, len); ny = wd_div(sy, len); nz = wd_div(sz, len);
    }
    normals[3u * (size_t)v] = nx;
    normals[3u * (size_t)v + 1u] = ny;
    normals[3u * (size_t)v + 2u] = nz;
}

inline dim3 per_item_grid(u64 n) { return dim3((u32)((n + MA_THREADS - 1u) / MA_THREADS)); }
inline u32 face_rows(u32 F) { return ceil_div(F, MA_FACE_TILE); }
inline u32 edge_rows(u32 S) { return (u32)(((u64)S + MA_PAIR_TILE - 1u) / MA_PAIR_TILE); }
inline u32 vertex_rows(u32 V) { return (u32)(((u64)V + MA_VERTEX_TILE) / MA_VERTEX_TILE); }   // (V + 1 threads' worth)

}  // namespace

// ---------------------------------------------------------------- the C ABI object (include/webdgs.h)
struct wdgs_mesh_adjacency {
    wdgs_device* dev = nullptr;
    KeySort sort;                       // reserved for 6 F slots
    ScanScratch vertex_scan;            // for the scan of degree[V + 1]
    DevMem<unsigned long long> keys;    // [6 F]
    DevMem<u32> neighbours, face_partial, edge_partial;   // [6 F] (E of them used), [rows of 1024 faces], [2 rows of 4096 slots]
    DevMem<u32> rows, degree, row_start, vertex_partial;   // [3 V], [V + 1], [V + 1], [3 rows of 2048 vertices]
    DevMem<float> pong;                 // [3 V]: the smoothing steps' second buffer
    DevMem<u32> totals;                 // MA_T_WORDS
    u32 capacity_v = 0, capacity_s = 0;
    bool counted = false, has_row_start = false;
    const void* faces = nullptr;
    u32 V = 0, F = 0, E = 0;
    u32 host[MA_T_WORDS] = {};
};

namespace {

// One wait on a call that grows: whichever of the two drains comes second -- this one or the sort's own -- finds the lanes idle
int adjacency_reserve(wdgs_mesh_adjacency* a, u32 V, u32 S) {
    wdgs_device* d = a->dev;
    if (V > a->capacity_v || S > a->capacity_s || !a->has_row_start) WDGS_CHECK_HIP(wdgs_sync_lanes(d));   // (nothing in flight may still read the blocks given back)
    if (V > a->capacity_v || !a->has_row_start) {
        a->capacity_v = 0;
        a->has_row_start = false;
        WDGS_TRY(a->rows.alloc((size_t)MA_R_PLANES * V, false, d->stream));
        WDGS_TRY(a->degree.alloc((size_t)V + 1u, false, d->stream));
        WDGS_TRY(a->row_start.alloc((size_t)V + 1u, false, d->stream));
        WDGS_TRY(a->pong.alloc(3 * (size_t)V, false, d->stream));
        WDGS_TRY(a->vertex_partial.alloc(3 * (size_t)vertex_rows(V), false, d->stream));
        WDGS_TRY(scan_scratch_create(&a->vertex_scan, V + 1u));
        a->capacity_v = V;
        a->has_row_start = true;
    }
    if (S > a->capacity_s) {
        a->capacity_s = 0;
        WDGS_TRY(a->keys.alloc(S, false, d->stream));
        WDGS_TRY(a->neighbours.alloc(S, false, d->stream));
        WDGS_TRY(a->face_partial.alloc(face_rows(S / 6u), false, d->stream));
        WDGS_TRY(a->edge_partial.alloc(2 * (size_t)edge_rows(S), false, d->stream));
        a->capacity_s = S;
    }
    return a->sort.reserve(d, S);
}

int launch_copy(wdgs_device* d, const void* in, void* out, size_t words) {
    if (words == 0u) return WDGS_OK;
    WDGS_LAUNCH(d, "adjacency_copy", ma_copy_kernel, per_item_grid(words), dim3(MA_THREADS), 0, static_cast<const u32*>(in), static_cast<u32*>(out), words);
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

}  // namespace

extern "C" int wdgs_mesh_adjacency_create(wdgs_device* dev, wdgs_mesh_adjacency** out) {
    WDGS_REQUIRE(dev && out, WDGS_E_INVALID, "wdgs_mesh_adjacency_create: null argument");
    WDGS_REQUIRE(!dev->capturing, WDGS_E_STATE, "wdgs_mesh_adjacency_create while recording a command buffer");
    auto a = std::make_unique<wdgs_mesh_adjacency>();
    a->dev = dev;
    WDGS_TRY(a->sort.create(dev));
    WDGS_TRY(a->totals.alloc(MA_T_WORDS, true, dev->stream));
    *out = a.release();
    return WDGS_OK;
}

extern "C" int wdgs_mesh_adjacency_destroy(wdgs_mesh_adjacency* a) {
    if (!a) return WDGS_OK;
    if (wdgs_device_alive(a->dev) && !a->dev->capturing) (void)wdgs_sync_lanes(a->dev);
    delete a;
    return WDGS_OK;
}

extern "C" int wdgs_mesh_adjacency_count(wdgs_mesh_adjacency* a, const void* faces_u32_dev, uint32_t num_faces, uint32_t num_vertices, uint32_t* directed_edges) {
    WDGS_REQUIRE(a && directed_edges, WDGS_E_INVALID, "wdgs_mesh_adjacency_count: null argument");
    a->counted = false;   // (a refused count leaves nothing to emit)
    *directed_edges = 0;
    WDGS_REQUIRE(num_vertices < (1u << 31) && (unsigned long long)num_faces * 6ull < (1ull << 32), WDGS_E_INVALID,
                 "meshAdjacency: %u vertices and %u faces: 2^31 vertices or 2^32 half-edges or more", num_vertices, num_faces);
    WDGS_REQUIRE(num_faces == 0 || faces_u32_dev, WDGS_E_INVALID, "wdgs_mesh_adjacency_count: null faces");
    WDGS_REQUIRE(((uintptr_t)faces_u32_dev & 3u) == 0u, WDGS_E_INVALID, "wdgs_mesh_adjacency_count: misaligned buffer");
    wdgs_device* d = a->dev;
    WDGS_REQUIRE(!d->capturing, WDGS_E_STATE, "meshAdjacency: the count waits for its totals and cannot be recorded into a command buffer");
    const u32 V = num_vertices, F = num_faces, S = 6u * F;
    const u32* faces = static_cast<const u32*>(faces_u32_dev);
    WDGS_TRY(adjacency_reserve(a, V, S));
    WDGS_CHECK_HIP(hipMemsetAsync(a->totals, 0, sizeof(u32) * MA_T_WORDS, d->stream));
    if (V != 0u) WDGS_CHECK_HIP(hipMemsetAsync(a->rows, 0, sizeof(u32) * MA_R_PLANES * (size_t)V, d->stream));
    if (S != 0u) {
        WDGS_LAUNCH(d, "adjacency_half_edge_keys", ma_half_edge_keys_kernel, dim3(face_rows(F)), dim3(MA_THREADS), 0, faces, F, V, a->keys.get(), a->face_partial.get());
        WDGS_CHECK_HIP(hipGetLastError());
        WDGS_TRY(a->sort.sort(d, a->keys, S, a->totals + MA_T_DISTINCT));
        WDGS_LAUNCH(d, "adjacency_edges", ma_edges_kernel, dim3(edge_rows(S)), dim3(MA_THREADS), 0, a->sort.view(a->keys), S, V, (const u32*)a->sort.flags,
                    (const u32*)a->sort.ids, a->neighbours.get(), a->rows.get(), a->edge_partial.get());
    }
    WDGS_LAUNCH(d, "adjacency_rows", ma_rows_kernel, dim3(vertex_rows(V)), dim3(MA_THREADS), 0, V, (const u32*)a->sort.flags, (const u32*)a->sort.ids,
                (const u32*)a->rows, a->degree.get(), a->vertex_partial.get());
    WDGS_LAUNCH(d, "adjacency_fold", ma_fold_kernel, dim3(1), dim3(MA_THREADS), 0, (const u32*)a->face_partial, S != 0u ? face_rows(F) : 0u, (const u32*)a->edge_partial,
                S != 0u ? edge_rows(S) : 0u, (const u32*)a->vertex_partial, vertex_rows(V), a->totals.get());
    WDGS_CHECK_HIP(hipGetLastError());
    WDGS_TRY(scan_exclusive_u32(d, &a->vertex_scan, a->degree, a->row_start, V + 1u, nullptr));
    WDGS_CHECK_HIP(hipMemcpyAsync(a->host, a->totals, sizeof(a->host), hipMemcpyDeviceToHost, d->stream));
    WDGS_CHECK_HIP(wdgs_sync_lanes(d));
    a->faces = faces_u32_dev;
    a->V = V;
    a->F = F;
    a->E = a->host[MA_T_DISTINCT] - (a->host[MA_T_INVALID] != 0u ? 1u : 0u);   // (the invalid faces' one key is no edge)
    a->counted = true;
    *directed_edges = a->E;
    return WDGS_OK;
}

extern "C" int wdgs_mesh_adjacency_emit(wdgs_mesh_adjacency* a, void* row_start_out_u32_dev, void* neighbours_out_u32_dev, void* boundary_out_u32_dev,
                                        uint32_t capacity_edges) {
    WDGS_REQUIRE(a, WDGS_E_INVALID, "wdgs_mesh_adjacency_emit: null argument");
    WDGS_REQUIRE(a->counted, WDGS_E_STATE, "meshAdjacency: no count precedes the emit");
    WDGS_REQUIRE(capacity_edges >= a->E, WDGS_E_CAPACITY, "meshAdjacency: %u directed edges, room for %u", a->E, capacity_edges);
    WDGS_REQUIRE((((uintptr_t)row_start_out_u32_dev | (uintptr_t)neighbours_out_u32_dev | (uintptr_t)boundary_out_u32_dev) & 3u) == 0u, WDGS_E_INVALID,
                 "wdgs_mesh_adjacency_emit: misaligned buffer");
    wdgs_device* d = a->dev;
    WDGS_LAUNCH(d, "adjacency_emit", ma_emit_kernel, per_item_grid(std::max<u64>((u64)a->V + 1u, a->E)), dim3(MA_THREADS), 0, a->V, a->E, (const u32*)a->row_start,
                (const u32*)a->neighbours, (const u32*)(a->rows.get() + (size_t)MA_R_BOUNDARY * a->V), static_cast<u32*>(row_start_out_u32_dev),
                static_cast<u32*>(neighbours_out_u32_dev), static_cast<u32*>(boundary_out_u32_dev));
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

extern "C" int wdgs_mesh_adjacency_smooth(wdgs_mesh_adjacency* a, const void* vertices_in_f32_dev, void* vertices_out_f32_dev, uint32_t num_vertices, uint32_t iterations,
                                          float lambda, float mu, uint32_t flags) {
    WDGS_REQUIRE(a, WDGS_E_INVALID, "wdgs_mesh_adjacency_smooth: null argument");
    WDGS_REQUIRE(std::isfinite(lambda) && std::isfinite(mu), WDGS_E_INVALID, "smoothMesh: lambda %g and mu %g must be finite", (double)lambda, (double)mu);
    WDGS_REQUIRE(iterations <= WDGS_SMOOTH_MAX_ITERATIONS, WDGS_E_INVALID, "smoothMesh: %u iterations, at most %u", iterations, WDGS_SMOOTH_MAX_ITERATIONS);
    WDGS_REQUIRE((flags & ~WDGS_SMOOTH_PIN_BOUNDARY) == 0u, WDGS_E_INVALID, "smoothMesh: unknown flags %#x", flags);
    WDGS_REQUIRE(a->counted && num_vertices == a->V, WDGS_E_STATE, "smoothMesh: no count of a mesh of %u vertices precedes it", num_vertices);
    WDGS_REQUIRE(a->V == 0 || (vertices_in_f32_dev && vertices_out_f32_dev), WDGS_E_INVALID, "wdgs_mesh_adjacency_smooth: null vertices");
    WDGS_REQUIRE((((uintptr_t)vertices_in_f32_dev | (uintptr_t)vertices_out_f32_dev) & 3u) == 0u, WDGS_E_INVALID, "wdgs_mesh_adjacency_smooth: misaligned buffer");
    if (a->V == 0) return WDGS_OK;
    wdgs_device* d = a->dev;
    const u32 V = a->V;
    const size_t words = 3 * (size_t)V;
    const u32 per_round = (lambda != 0.f ? 1u : 0u) + (mu != 0.f ? 1u : 0u), steps = iterations * per_round;
    const float* in = static_cast<const float*>(vertices_in_f32_dev);
    float* out = static_cast<float*>(vertices_out_f32_dev);
    if (steps == 0u) return in == out ? WDGS_OK : launch_copy(d, in, out, words);
    // The last step writes `out`, the one before it the object's buffer, and so on backwards.  The first step would then read and write `out` where the steps
    // are odd in number and the caller smooths in place: it reads a copy instead.
    const float* src = in;
    if ((steps & 1u) != 0u && in == out) {
        WDGS_TRY(launch_copy(d, in, a->pong, words));
        src = a->pong;
    }
    const u32* boundary = a->rows.get() + (size_t)MA_R_BOUNDARY * V;
    u32 k = 0;
    for (u32 it = 0; it < iterations; it++) {
        for (u32 half = 0; half < 2u; half++) {
            const float w = half == 0u ? lambda : mu;
            if (w == 0.f) continue;
            float* dst = ((steps - 1u - k) & 1u) == 0u ? out : a->pong.get();
            WDGS_LAUNCH(d, "adjacency_smooth_step", ma_smooth_step_kernel, per_item_grid(V), dim3(MA_THREADS), 0, src, dst, V, (const u32*)a->row_start,
                        (const u32*)a->neighbours, boundary, flags & WDGS_SMOOTH_PIN_BOUNDARY, w);
            src = dst;
            k++;
        }
    }
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

extern "C" int wdgs_mesh_adjacency_normals(wdgs_mesh_adjacency* a, const void* vertices_f32_dev, const void* faces_u32_dev, uint32_t num_vertices, uint32_t num_faces,
                                           void* normals_out_f32_dev) {
    WDGS_REQUIRE(a, WDGS_E_INVALID, "wdgs_mesh_adjacency_normals: null argument");
    WDGS_REQUIRE(a->counted && num_vertices == a->V && num_faces == a->F && faces_u32_dev == a->faces, WDGS_E_STATE,
                 "vertexNormals: no count of these faces over %u vertices precedes it", num_vertices);
    WDGS_REQUIRE(a->V == 0 || (vertices_f32_dev && normals_out_f32_dev), WDGS_E_INVALID, "wdgs_mesh_adjacency_normals: null vertices or normals");
    WDGS_REQUIRE((((uintptr_t)vertices_f32_dev | (uintptr_t)normals_out_f32_dev) & 3u) == 0u, WDGS_E_INVALID, "wdgs_mesh_adjacency_normals: misaligned buffer");
    if (a->V == 0) return WDGS_OK;
    wdgs_device* d = a->dev;
    WDGS_LAUNCH(d, "adjacency_vertex_normals", ma_vertex_normals_kernel, per_item_grid(a->V), dim3(MA_THREADS), 0, static_cast<const float*>(vertices_f32_dev),
                static_cast<const u32*>(faces_u32_dev), a->V, a->sort.view(a->keys), (const u32*)a->rows, static_cast<float*>(normals_out_f32_dev));
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

extern "C" int wdgs_mesh_adjacency_stats(const wdgs_mesh_adjacency* a, uint32_t* directed_edges, uint32_t* edges, uint32_t* boundary_edges, uint32_t* non_manifold_edges,
                                         uint32_t* invalid_faces, uint32_t* boundary_vertices, uint32_t* isolated_vertices, uint32_t* max_degree) {
    WDGS_REQUIRE(a, WDGS_E_INVALID, "wdgs_mesh_adjacency_stats: null argument");
    WDGS_REQUIRE(a->counted, WDGS_E_STATE, "meshAdjacency: no count precedes the read of its statistics");
    if (directed_edges) *directed_edges = a->E;
    if (edges) *edges = a->E / 2u;
    if (boundary_edges) *boundary_edges = a->host[MA_T_BOUNDARY_EDGES];
    if (non_manifold_edges) *non_manifold_edges = a->host[MA_T_NON_MANIFOLD];
    if (invalid_faces) *invalid_faces = a->host[MA_T_INVALID];
    if (boundary_vertices) *boundary_vertices = a->host[MA_T_BOUNDARY_VERTICES];
    if (isolated_vertices) *isolated_vertices = a->host[MA_T_ISOLATED];
    if (max_degree) *max_degree = a->host[MA_T_MAX_DEGREE];
    return WDGS_OK;
}
