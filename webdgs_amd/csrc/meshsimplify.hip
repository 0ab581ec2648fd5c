// Mesh simplification by vertex clustering on the device (no counterpart in the reference, which renders colour only).
//
// Every vertex falls into a cell of a uniform grid; the distinct cells that hold a vertex are the clusters, numbered in ascending key order by the library's
// stable u64 sort (KeySort::rank, keysort.hip, with S = V).  A cluster's representative is the integer mean of its vertices' 16-bit sub-cell
// offsets, its colour the integer mean of their bytes: only integers are ever summed, so no result depends on the order in which threads ran.  Faces are
// classified, rotated so that their smallest cluster leads, and the duplicates among them found by two more sorts (S = F): the rank of (b, c) feeds the key
// (a, rank), and -- the sort being stable -- the head of a run of equal second keys is the lowest face index with that triple.  Kept faces flag their
// clusters; two scans number the emitted vertices and faces; the emit gathers.
//
// Section 16's and 17's rule holds: no spin-wait, no inter-workgroup flag, no look-back, no grid barrier, no float atomics.  The only global atomics are
// ms_accumulate's integer adds onto the clusters' sums, which commute; everything else reads what earlier launches wrote, with plain loads.
#include <cmath>
#include <memory>

#include "launch.h"

namespace {

typedef unsigned long long u64;

constexpr u32 MS_THREADS = 256;
constexpr u32 MS_WAVES = MS_THREADS / 64;
constexpr u64 MS_NO_KEY = ~0ull;
constexpr u32 MS_NONE = 0xFFFFFFFFu;
constexpr u32 MS_CELLS = 1u << 21;              // cells per axis
constexpr u32 MS_STEPS = 16;                    // steps of 64 vertices a wave of ms_accumulate sums before it has to touch memory
constexpr u32 MS_ACC_TILE = MS_THREADS * MS_STEPS;   // 4096 vertices per workgroup
constexpr u32 MS_ACC_WORDS = 8;                 // per cluster, u64: Qx, Qy, Qz, n, and the four colour sums
constexpr u32 MS_FACE_ROUNDS = 4;               // faces per thread of ms_face_keys: its workgroup leaves one row of class counts per 1024 faces
constexpr u32 MS_FACE_TILE = MS_THREADS * MS_FACE_ROUNDS;
// The totals block, u32 words: distinct keys (the outside key included), emitted vertices, kept faces, the three class counts ms_fold leaves, 1 when the
// last distinct key is the outside key, the two sorts' distinct face keys (unused by the host)
constexpr u32 MS_T_DISTINCT = 0, MS_T_VERTICES = 1, MS_T_FACES = 2, MS_T_INVALID = 3, MS_T_OUTSIDE = 4, MS_T_COLLAPSED = 5, MS_T_HAS_OUTSIDE = 6, MS_T_SPARE = 7,
              MS_T_WORDS = 8;

struct MsGrid { float origin[3]; float inv, cell; };

// t = (p - origin) * inv and c = floorf(t), each operation rounded once; true when t is finite and 0 <= c < 2^21
__device__ __forceinline__ bool cell_of(float p, float origin, float inv, float& t, float& c) {
    const float d = p - origin;
    t = d * inv;
    c = floorf(t);
    return (__float_as_uint(t) & 0x7F800000u) != 0x7F800000u && c >= 0.f && c < (float)MS_CELLS;
}

// The sum of x over the wave, in every lane
__device__ __forceinline__ u32 wave_sum(u32 x) {
#pragma unroll
    for (u32 d = 32; d >= 1; d >>= 1) x += (u32)__shfl_xor((int)x, (int)d, 64);
    return x;
}

// keys[v]: the cell key of vertex v, or MS_NO_KEY outside the grid
__global__ __launch_bounds__(MS_THREADS) void ms_cell_keys_kernel(const float* __restrict__ vertices, u32 V, MsGrid g, u64* __restrict__ keys) {
    const u32 v = blockIdx.x * MS_THREADS + threadIdx.x;
    if (v >= V) return;
    u64 key = 0ull;
    bool inside = true;
#pragma unroll
    for (u32 a = 0; a < 3u; a++) {
        float t, c;
        inside = cell_of(vertices[3u * (size_t)v + a], g.origin[a], g.inv, t, c) && inside;
        key |= (u64)(inside ? (u32)c : 0u) << (21u * a);
    }
    keys[v] = inside ? key : MS_NO_KEY;
}

// What one cluster gathers: five words a lane or a wave step can hold in 32 bits (64 * 65535 and 64 * 255 fit), widened when they are added to a run
struct MsSums {
    u64 q[3], n, c[4];
    __device__ __forceinline__ void clear() { q[0] = q[1] = q[2] = n = c[0] = c[1] = c[2] = c[3] = 0ull; }
    __device__ __forceinline__ void add(u32 qx, u32 qy, u32 qz, u32 count, u32 c01, u32 c23) {
        q[0] += qx; q[1] += qy; q[2] += qz; n += count;
        c[0] += c01 & 0xFFFFu; c[1] += c01 >> 16; c[2] += c23 & 0xFFFFu; c[3] += c23 >> 16;
    }
    __device__ __forceinline__ void add(const MsSums& o) {
#pragma unroll
        for (u32 k = 0; k < 3u; k++) q[k] += o.q[k];
        n += o.n;
#pragma unroll
        for (u32 k = 0; k < 4u; k++) c[k] += o.c[k];
    }
};

__device__ __forceinline__ void ms_flush(u64* __restrict__ acc, u32 cluster, const MsSums& s, bool with_colours) {
    u64* row = acc + (size_t)cluster * MS_ACC_WORDS;
#pragma unroll
    for (u32 k = 0; k < 3u; k++) atomicAdd(row + k, s.q[k]);
    atomicAdd(row + 3, s.n);
    if (with_colours) {
#pragma unroll
        for (u32 k = 0; k < 4u; k++) atomicAdd(row + 4 + k, s.c[k]);
    }
}

// acc[cluster]: the sums of the sub-cell offsets q = u32((t - c) * 65536) per axis, the vertex count and the colour bytes' sums, over the cluster's vertices.
// A workgroup owns 4096 consecutive vertices and wave w of it 1024, as 16 steps of 64.  A step whose inside vertices share one cluster -- the usual case, TSDF
// vertices arrive nearly key-sorted -- is summed by shuffles and joins the wave's RUN, held in registers, while the cluster stays the same; a run is added to
// memory (integer atomics, one lane) only when the cluster changes.  A mixed step closes the run; its lanes find their equals with ballots (match_digit), a
// lane alone in its cluster adds its own values, and every larger group is summed by shuffles and added by its lowest lane.  At the end the four waves' open
// runs meet in LDS and thread 0 joins neighbours of one cluster before adding them: with every vertex in one cell that is one set of adds per 4096 vertices.
__global__ __launch_bounds__(MS_THREADS) void ms_accumulate_kernel(const float* __restrict__ vertices, const u32* __restrict__ colours, const u32* __restrict__ rank, u32 V,
                                                                   MsGrid g, u64* __restrict__ acc) {
    __shared__ u32 tail_cluster[MS_WAVES];
    __shared__ u64 tail_sums[MS_WAVES][MS_ACC_WORDS];
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const bool with_colours = colours != nullptr;
    const u64 first = (u64)blockIdx.x * MS_ACC_TILE + (u64)wave * (MS_STEPS * 64u) + lane;
    u32 cur = MS_NONE;   // (uniform in the wave, like run)
    MsSums run;
    run.clear();
    for (u32 step = 0; step < MS_STEPS; step++) {
        const u64 v = first + step * 64u;
        bool valid = v < (u64)V;
        u32 q[3] = {0u, 0u, 0u}, c01 = 0u, c23 = 0u, r = MS_NONE;
        if (valid) {
#pragma unroll
            for (u32 a = 0; a < 3u; a++) {
                float t, c;
                valid = cell_of(vertices[3u * (size_t)v + a], g.origin[a], g.inv, t, c) && valid;
                const float frac = t - c;               // exact
                q[a] = (u32)(frac * 65536.0f);          // truncates
            }
        }
        if (valid) {
            r = rank[v];
            if (with_colours) {
                const u32 w = colours[v];
                c01 = (w & 0xFFu) | ((w & 0xFF00u) << 8);
                c23 = ((w >> 16) & 0xFFu) | ((w >> 24) << 16);
            }
        } else {
            q[0] = q[1] = q[2] = 0u;
        }
        const u64 vm = __ballot(valid);
        if (vm == 0ull) continue;   // (uniform in the wave; the barrier below is outside the loop)
        const u32 r0 = (u32)__shfl((int)r, __ffsll((long long)vm) - 1, 64);
        if (__ballot(valid && r != r0) == 0ull) {
            const u32 sx = wave_sum(q[0]), sy = wave_sum(q[1]), sz = wave_sum(q[2]), s01 = wave_sum(c01), s23 = wave_sum(c23);
            if (r0 != cur) {
                if (cur != MS_NONE && lane == 0u) ms_flush(acc, cur, run, with_colours);
                cur = r0;
                run.clear();
            }
            run.add(sx, sy, sz, (u32)__popcll(vm), s01, s23);
            continue;
        }
        if (cur != MS_NONE && lane == 0u) ms_flush(acc, cur, run, with_colours);
        cur = MS_NONE;
        run.clear();
        const u64 m = match_digit<32>(r, vm);   // (meaningful in the valid lanes)
        const bool alone = valid && __popcll(m) == 1;
        if (alone) {
            MsSums s;
            s.clear();
            s.add(q[0], q[1], q[2], 1u, c01, c23);
            ms_flush(acc, r, s, with_colours);
        }
        u64 leaders = __ballot(valid && !alone && lanes_below(m) == 0u);
        while (leaders != 0ull) {   // (uniform in the wave)
            const int l = __ffsll((long long)leaders) - 1;
            leaders &= leaders - 1ull;
            const u64 gm = ((u64)(u32)__shfl((int)(u32)(m >> 32), l, 64) << 32) | (u64)(u32)__shfl((int)(u32)m, l, 64);
            const bool in = ((gm >> lane) & 1ull) != 0ull;
            const u32 sx = wave_sum(in ? q[0] : 0u), sy = wave_sum(in ? q[1] : 0u), sz = wave_sum(in ? q[2] : 0u), s01 = wave_sum(in ? c01 : 0u),
                      s23 = wave_sum(in ? c23 : 0u);
            if ((int)lane == l) {
                MsSums s;
                s.clear();
                s.add(sx, sy, sz, (u32)__popcll(gm), s01, s23);
                ms_flush(acc, r, s, with_colours);
            }
        }
    }
    if (lane == 0u) {
        tail_cluster[wave] = cur;
        u64* t = tail_sums[wave];
        t[0] = run.q[0]; t[1] = run.q[1]; t[2] = run.q[2]; t[3] = run.n;
        t[4] = run.c[0]; t[5] = run.c[1]; t[6] = run.c[2]; t[7] = run.c[3];
    }
    __syncthreads();
    if (threadIdx.x != 0u) return;
    u32 pending = MS_NONE;
    MsSums sum;
    sum.clear();
    for (u32 w = 0; w < MS_WAVES; w++) {
        const u32 cl = tail_cluster[w];
        if (cl == MS_NONE) continue;
        if (cl != pending) {
            if (pending != MS_NONE) ms_flush(acc, pending, sum, with_colours);
            pending = cl;
            sum.clear();
        }
        MsSums s;
        const u64* t = tail_sums[w];
        s.q[0] = t[0]; s.q[1] = t[1]; s.q[2] = t[2]; s.n = t[3];
        s.c[0] = t[4]; s.c[1] = t[5]; s.c[2] = t[6]; s.c[3] = t[7];
        sum.add(s);
    }
    if (pending != MS_NONE) ms_flush(acc, pending, sum, with_colours);
}

// One thread per distinct key that is a cluster: the representative origin + (f32(c) + (f32(Qm) + 0.5) * 2^-16) * cell_size, Qm = (2 Q + n) / (2 n), and the
// colour (2 sum + n) / (2 n) per byte
__global__ __launch_bounds__(MS_THREADS) void ms_finalize_kernel(const u64* __restrict__ cluster_keys, const u32* __restrict__ totals, const u64* __restrict__ acc, MsGrid g,
                                                                 bool with_colours, float* __restrict__ positions, u32* __restrict__ colours) {
    const u32 r = blockIdx.x * MS_THREADS + threadIdx.x;
    if (r >= totals[MS_T_DISTINCT]) return;
    const u64 key = cluster_keys[r];
    if (key == MS_NO_KEY) return;
    const u64* row = acc + (size_t)r * MS_ACC_WORDS;
    const u64 n = row[3];   // (>= 1: the key came from a vertex)
#pragma unroll
    for (u32 a = 0; a < 3u; a++) {
        const u32 c = (u32)(key >> (21u * a)) & (MS_CELLS - 1u);
        const u64 qm = (2ull * row[a] + n) / (2ull * n);
        const float h = (float)(u32)qm + 0.5f;
        const float f = h * (1.0f / 65536.0f);
        const float s = (float)c + f;
        const float m = s * g.cell;
        positions[3u * (size_t)r + a] = g.origin[a] + m;
    }
    if (with_colours) {
        u32 w = 0u;
#pragma unroll
        for (u32 k = 0; k < 4u; k++) w |= (u32)((2ull * row[4u + k] + n) / (2ull * n)) << (8u * k);
        colours[r] = w;
    }
}

// One thread per face, four faces in turn.  The class: invalid (an index >= V, never read as an address), outside (a corner outside the grid), collapsed (two
// corners in one cluster), else a candidate.  lead[f] = the smallest cluster a of the candidate's rotated triple (a, b, c), keys[f] = b * 2^32 | c; a dropped
// face gets MS_NONE and MS_NO_KEY.  iota[f] = f (what the second sort's emit gathers).  partial[3 g ..]: the workgroup's faces of the three classes.
__global__ __launch_bounds__(MS_THREADS) void ms_face_keys_kernel(const u32* __restrict__ faces, u32 F, u32 V, const u64* __restrict__ vertex_keys,
                                                                  const u32* __restrict__ rank, u64* __restrict__ keys, u32* __restrict__ lead, u32* __restrict__ iota,
                                                                  u32* __restrict__ partial) {
    __shared__ u32 counts[MS_WAVES][3];
    u32 mine[3] = {0u, 0u, 0u};
    for (u32 round = 0; round < MS_FACE_ROUNDS; round++) {
        const u64 f = (u64)blockIdx.x * MS_FACE_TILE + round * MS_THREADS + threadIdx.x;
        if (f >= (u64)F) break;
        const u32 i0 = faces[3u * f], i1 = faces[3u * f + 1u], i2 = faces[3u * f + 2u];
        u64 key = MS_NO_KEY;
        u32 a = MS_NONE;
        if (i0 >= V || i1 >= V || i2 >= V) {
            mine[0]++;
        } else if (vertex_keys[i0] == MS_NO_KEY || vertex_keys[i1] == MS_NO_KEY || vertex_keys[i2] == MS_NO_KEY) {
            mine[1]++;
        } else {
            const u32 r0 = rank[i0], r1 = rank[i1], r2 = rank[i2];
            if (r0 == r1 || r1 == r2 || r0 == r2) {
                mine[2]++;
            } else if (r0 < r1 && r0 < r2) {
                a = r0; key = ((u64)r1 << 32) | r2;
            } else if (r1 < r2) {
                a = r1; key = ((u64)r2 << 32) | r0;
            } else {
                a = r2; key = ((u64)r0 << 32) | r1;
            }
        }
        keys[f] = key;
        lead[f] = a;
        iota[f] = (u32)f;
    }
#pragma unroll
    for (u32 k = 0; k < 3u; k++) mine[k] = wave_sum(mine[k]);
    if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
        for (u32 k = 0; k < 3u; k++) counts[threadIdx.x >> 6][k] = mine[k];
    }
    __syncthreads();
    if (threadIdx.x < 3u) {
        u32 n = 0u;
#pragma unroll
        for (u32 w = 0; w < MS_WAVES; w++) n += counts[w][threadIdx.x];
        partial[3u * blockIdx.x + threadIdx.x] = n;
    }
}

// One workgroup: folds the rows of class counts into the totals block, and notes whether the last distinct vertex key is the outside key
__global__ __launch_bounds__(MS_THREADS) void ms_fold_kernel(const u32* __restrict__ partial, u32 rows, const u64* __restrict__ cluster_keys, u32* __restrict__ totals) {
    __shared__ u32 counts[MS_WAVES][3];
    u32 mine[3] = {0u, 0u, 0u};
    for (u32 g = threadIdx.x; g < rows; g += MS_THREADS) {
#pragma unroll
        for (u32 k = 0; k < 3u; k++) mine[k] += partial[3u * g + k];
    }
#pragma unroll
    for (u32 k = 0; k < 3u; k++) mine[k] = wave_sum(mine[k]);
    if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
        for (u32 k = 0; k < 3u; k++) counts[threadIdx.x >> 6][k] = mine[k];
    }
    __syncthreads();
    if (threadIdx.x < 3u) {
        u32 n = 0u;
#pragma unroll
        for (u32 w = 0; w < MS_WAVES; w++) n += counts[w][threadIdx.x];
        totals[MS_T_INVALID + threadIdx.x] = n;
    }
    if (threadIdx.x == 3u) {
        const u32 d = totals[MS_T_DISTINCT];
        totals[MS_T_HAS_OUTSIDE] = (d != 0u && cluster_keys[d - 1u] == MS_NO_KEY) ? 1u : 0u;
    }
}

// keys[f] = lead[f] * 2^32 | rank1[f] for a candidate (rank1: the rank of its first key); a dropped face keeps MS_NO_KEY
__global__ __launch_bounds__(MS_THREADS) void ms_face_keys2_kernel(const u32* __restrict__ lead, const u32* __restrict__ rank1, u32 F, u64* __restrict__ keys) {
    const u32 f = blockIdx.x * MS_THREADS + threadIdx.x;
    if (f >= F) return;
    const u32 a = lead[f];
    keys[f] = a == MS_NONE ? MS_NO_KEY : (((u64)a << 32) | rank1[f]);
}

// A candidate is kept when it is the lowest face of its triple: head_face[rank2[f]] == f.  Kept faces flag their three clusters (racing stores of 1).
__global__ __launch_bounds__(MS_THREADS) void ms_mark_kernel(const u32* __restrict__ faces, u32 F, const u32* __restrict__ lead, const u32* __restrict__ rank2,
                                                             const u32* __restrict__ head_face, const u32* __restrict__ rank, u32* __restrict__ face_flags,
                                                             u32* __restrict__ cluster_flags) {
    const u32 f = blockIdx.x * MS_THREADS + threadIdx.x;
    if (f >= F) return;
    const bool keep = lead[f] != MS_NONE && head_face[rank2[f]] == f;
    face_flags[f] = keep ? 1u : 0u;
    if (!keep) return;
#pragma unroll
    for (u32 k = 0; k < 3u; k++) cluster_flags[rank[faces[3u * (size_t)f + k]]] = 1u;   // (a candidate's indices are < V)
}

// Thread i as distinct key i: a flagged cluster writes its vertex.  Thread i as input vertex i: vertex_cluster[i]
__global__ __launch_bounds__(MS_THREADS) void ms_emit_vertices_kernel(u32 V, const u32* __restrict__ totals, const u32* __restrict__ cluster_flags,
                                                                      const u32* __restrict__ cluster_offsets, const u64* __restrict__ cluster_keys,
                                                                      const float* __restrict__ positions, const u32* __restrict__ colours,
                                                                      const u64* __restrict__ vertex_keys, const u32* __restrict__ rank, float* __restrict__ vertices_out,
                                                                      u32* __restrict__ colours_out, u64* __restrict__ keys_out, u32* __restrict__ vertex_cluster) {
    const u32 i = blockIdx.x * MS_THREADS + threadIdx.x;
    if (i >= V) return;
    if (i < totals[MS_T_DISTINCT] && cluster_flags[i] != 0u) {
        const u32 v = cluster_offsets[i];
#pragma unroll
        for (u32 a = 0; a < 3u; a++) vertices_out[3u * (size_t)v + a] = positions[3u * (size_t)i + a];
        if (colours_out) colours_out[v] = colours[i];
        if (keys_out) keys_out[v] = cluster_keys[i];
    }
    if (vertex_cluster) {
        u32 out = MS_NONE;
        if (vertex_keys[i] != MS_NO_KEY) {
            const u32 r = rank[i];
            if (cluster_flags[r] != 0u) out = cluster_offsets[r];
        }
        vertex_cluster[i] = out;
    }
}

__global__ __launch_bounds__(MS_THREADS) void ms_emit_faces_kernel(const u32* __restrict__ faces, u32 F, const u32* __restrict__ face_flags, const u32* __restrict__ face_offsets,
                                                                   const u32* __restrict__ rank, const u32* __restrict__ cluster_offsets, u32* __restrict__ faces_out,
                                                                   u32* __restrict__ face_map) {
    const u32 f = blockIdx.x * MS_THREADS + threadIdx.x;
    if (f >= F || face_flags[f] == 0u) return;
    const u32 j = face_offsets[f];
#pragma unroll
    for (u32 k = 0; k < 3u; k++) faces_out[3u * (size_t)j + k] = cluster_offsets[rank[faces[3u * (size_t)f + k]]];
    if (face_map) face_map[j] = f;
}

inline dim3 per_item_grid(u32 n) { return dim3(ceil_div(n, MS_THREADS)); }

}  // namespace

// ---------------------------------------------------------------- launchers
int launch_simplify_cell_keys(wdgs_device* dev, const float* vertices, u32 V, const float origin[3], float inv, float cell_size, unsigned long long* keys) {
    const MsGrid g{{origin[0], origin[1], origin[2]}, inv, cell_size};
    WDGS_LAUNCH(dev, "simplify_cell_keys", ms_cell_keys_kernel, per_item_grid(V), dim3(MS_THREADS), 0, vertices, V, g, keys);
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

int launch_simplify_accumulate(wdgs_device* dev, const float* vertices, const u32* colours, const u32* rank, u32 V, const float origin[3], float inv, float cell_size,
                               unsigned long long* acc) {
    const MsGrid g{{origin[0], origin[1], origin[2]}, inv, cell_size};
    WDGS_CHECK_HIP(hipMemsetAsync(acc, 0, sizeof(u64) * MS_ACC_WORDS * (size_t)V, dev->stream));
    WDGS_LAUNCH(dev, "simplify_accumulate", ms_accumulate_kernel, dim3(ceil_div(V, MS_ACC_TILE)), dim3(MS_THREADS), 0, vertices, colours, rank, V, g, acc);
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

int launch_simplify_finalize(wdgs_device* dev, const unsigned long long* cluster_keys, const u32* totals, const unsigned long long* acc, u32 V, const float origin[3],
                             float inv, float cell_size, bool with_colours, float* positions, u32* colours) {
    const MsGrid g{{origin[0], origin[1], origin[2]}, inv, cell_size};
    WDGS_LAUNCH(dev, "simplify_finalize", ms_finalize_kernel, per_item_grid(V), dim3(MS_THREADS), 0, (const u64*)cluster_keys, totals, (const u64*)acc, g, with_colours,
                positions, colours);
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

u32 simplify_partial_rows(u32 F) { return ceil_div(F, MS_FACE_TILE); }

int launch_simplify_face_keys(wdgs_device* dev, const u32* faces, u32 F, u32 V, const unsigned long long* vertex_keys, const u32* rank, unsigned long long* keys, u32* lead,
                              u32* iota, u32* partial) {
    WDGS_LAUNCH(dev, "simplify_face_keys", ms_face_keys_kernel, dim3(simplify_partial_rows(F)), dim3(MS_THREADS), 0, faces, F, V, (const u64*)vertex_keys, rank, keys, lead,
                iota, partial);
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

int launch_simplify_fold(wdgs_device* dev, const u32* partial, u32 rows, const unsigned long long* cluster_keys, u32* totals) {
    WDGS_LAUNCH(dev, "simplify_fold", ms_fold_kernel, dim3(1), dim3(MS_THREADS), 0, partial, rows, (const u64*)cluster_keys, totals);
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

int launch_simplify_face_keys2(wdgs_device* dev, const u32* lead, const u32* rank1, u32 F, unsigned long long* keys) {
    WDGS_LAUNCH(dev, "simplify_face_keys2", ms_face_keys2_kernel, per_item_grid(F), dim3(MS_THREADS), 0, lead, rank1, F, keys);
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

int launch_simplify_mark(wdgs_device* dev, const u32* faces, u32 F, u32 V, const u32* lead, const u32* rank2, const u32* head_face, const u32* rank, u32* face_flags,
                         u32* cluster_flags) {
    WDGS_CHECK_HIP(hipMemsetAsync(cluster_flags, 0, sizeof(u32) * (size_t)V, dev->stream));
    WDGS_LAUNCH(dev, "simplify_mark", ms_mark_kernel, per_item_grid(F), dim3(MS_THREADS), 0, faces, F, lead, rank2, head_face, rank, face_flags, cluster_flags);
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

int launch_simplify_emit(wdgs_device* dev, const u32* faces, u32 F, u32 V, const u32* totals, const u32* cluster_flags, const u32* cluster_offsets,
                         const unsigned long long* cluster_keys, const float* positions, const u32* colours, const unsigned long long* vertex_keys, const u32* rank,
                         const u32* face_flags, const u32* face_offsets, float* vertices_out, u32* colours_out, unsigned long long* keys_out, u32* faces_out, u32* face_map,
                         u32* vertex_cluster) {
    WDGS_LAUNCH(dev, "simplify_emit_vertices", ms_emit_vertices_kernel, per_item_grid(V), dim3(MS_THREADS), 0, V, totals, cluster_flags, cluster_offsets,
                (const u64*)cluster_keys, positions, colours, (const u64*)vertex_keys, rank, vertices_out, colours_out, keys_out, vertex_cluster);
    if (F != 0u) {
        WDGS_LAUNCH(dev, "simplify_emit_faces", ms_emit_faces_kernel, per_item_grid(F), dim3(MS_THREADS), 0, faces, F, face_flags, face_offsets, rank, cluster_offsets,
                    faces_out, face_map);
    }
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

// ---------------------------------------------------------------- the C ABI object (include/webdgs.h)
struct wdgs_mesh_simplifier {
    wdgs_device* dev = nullptr;
    KeySort sort;                                                // reserved for V and for F: the three sorts use it in turn
    // per vertex [V]
    DevMem<unsigned long long> vertex_keys, cluster_keys, acc;   // acc: [8 V]
    DevMem<u32> rank, cluster_colours, cluster_flags, cluster_offsets;
    DevMem<float> cluster_positions;                             // [3 V]
    // per face [F]
    DevMem<unsigned long long> face_keys;
    DevMem<u32> lead, face_rank, iota, head_face, face_flags, face_offsets, partial;
    DevMem<u32> totals;                                          // MS_T_WORDS
    u32 capacity_v = 0, capacity_f = 0;
    bool counted = false;
    const void *vertices = nullptr, *faces = nullptr, *colours = nullptr;
    u32 V = 0, F = 0;
    u32 clusters = 0, vertices_out = 0, faces_out = 0, invalid = 0, outside = 0, collapsed = 0, duplicate = 0;
};

namespace {

// One wait on a call that grows: whichever of the two drains comes second -- this one or the sort's own -- finds the lanes idle, no launch lying between them
int simplifier_reserve(wdgs_mesh_simplifier* s, u32 V, u32 F) {
    wdgs_device* d = s->dev;
    if (V > s->capacity_v || F > s->capacity_f) WDGS_CHECK_HIP(wdgs_sync_lanes(d));   // (nothing in flight may still read the blocks given back)
    if (V > s->capacity_v) {
        s->capacity_v = 0;
        WDGS_TRY(s->vertex_keys.alloc(V, false, d->stream));
        WDGS_TRY(s->cluster_keys.alloc(V, false, d->stream));
        WDGS_TRY(s->acc.alloc((size_t)MS_ACC_WORDS * V, false, d->stream));
        WDGS_TRY(s->rank.alloc(V, false, d->stream));
        WDGS_TRY(s->cluster_colours.alloc(V, false, d->stream));
        WDGS_TRY(s->cluster_flags.alloc(V, false, d->stream));
        WDGS_TRY(s->cluster_offsets.alloc(V, false, d->stream));
        WDGS_TRY(s->cluster_positions.alloc(3 * (size_t)V, false, d->stream));
        s->capacity_v = V;
    }
    if (F > s->capacity_f) {
        s->capacity_f = 0;
        WDGS_TRY(s->face_keys.alloc(F, false, d->stream));
        WDGS_TRY(s->lead.alloc(F, false, d->stream));
        WDGS_TRY(s->face_rank.alloc(F, false, d->stream));
        WDGS_TRY(s->iota.alloc(F, false, d->stream));
        WDGS_TRY(s->head_face.alloc(F, false, d->stream));
        WDGS_TRY(s->face_flags.alloc(F, false, d->stream));
        WDGS_TRY(s->face_offsets.alloc(F, false, d->stream));
        WDGS_TRY(s->partial.alloc(3 * (size_t)simplify_partial_rows(F), false, d->stream));
        s->capacity_f = F;
    }
    return s->sort.reserve(d, V, F);
}

}  // namespace

extern "C" int wdgs_mesh_simplifier_create(wdgs_device* dev, wdgs_mesh_simplifier** out) {
    WDGS_REQUIRE(dev && out, WDGS_E_INVALID, "wdgs_mesh_simplifier_create: null argument");
    WDGS_REQUIRE(!dev->capturing, WDGS_E_STATE, "wdgs_mesh_simplifier_create while recording a command buffer");
    auto s = std::make_unique<wdgs_mesh_simplifier>();
    s->dev = dev;
    WDGS_TRY(s->sort.create(dev));
    WDGS_TRY(s->totals.alloc(MS_T_WORDS, true, dev->stream));
    *out = s.release();
    return WDGS_OK;
}

extern "C" int wdgs_mesh_simplifier_destroy(wdgs_mesh_simplifier* s) {
    if (!s) return WDGS_OK;
    if (wdgs_device_alive(s->dev) && !s->dev->capturing) (void)wdgs_sync_lanes(s->dev);
    delete s;
    return WDGS_OK;
}

extern "C" int wdgs_mesh_simplifier_count(wdgs_mesh_simplifier* s, const void* vertices_f32_dev, uint32_t num_vertices, const void* faces_u32_dev, uint32_t num_faces,
                                          const void* colours_rgba8_dev, const float* origin, float cell_size, uint32_t* vertices_out, uint32_t* faces_out) {
    WDGS_REQUIRE(s && origin && vertices_out && faces_out, WDGS_E_INVALID, "wdgs_mesh_simplifier_count: null argument");
    s->counted = false;   // (a refused count leaves nothing to emit)
    *vertices_out = *faces_out = 0;
    WDGS_REQUIRE(num_vertices < (1u << 31) && num_faces < (1u << 31), WDGS_E_INVALID, "simplifyMesh: %u vertices and %u faces: 2^31 or more", num_vertices, num_faces);
    WDGS_REQUIRE((num_vertices == 0 || vertices_f32_dev) && (num_faces == 0 || faces_u32_dev), WDGS_E_INVALID, "wdgs_mesh_simplifier_count: null vertices or faces");
    WDGS_REQUIRE((((uintptr_t)vertices_f32_dev | (uintptr_t)faces_u32_dev | (uintptr_t)colours_rgba8_dev) & 3u) == 0u, WDGS_E_INVALID,
                 "wdgs_mesh_simplifier_count: misaligned buffer");
    WDGS_REQUIRE(std::isfinite(origin[0]) && std::isfinite(origin[1]) && std::isfinite(origin[2]), WDGS_E_INVALID, "simplifyMesh: the origin is not finite");
    WDGS_REQUIRE(std::isfinite(cell_size) && cell_size > 0.f, WDGS_E_INVALID, "simplifyMesh: the cell size %g is not finite and positive", (double)cell_size);
    wdgs_device* d = s->dev;
    WDGS_REQUIRE(!d->capturing, WDGS_E_STATE, "simplifyMesh: the count waits for its totals and cannot be recorded into a command buffer");
    const u32 V = num_vertices, F = num_faces;
    const float inv = 1.0f / cell_size;   // formed once, here: the kernels never divide floats
    u32 host[MS_T_WORDS] = {};
    if (V == 0u) {
        host[MS_T_INVALID] = F;   // (every index is >= V)
    } else {
        WDGS_TRY(simplifier_reserve(s, V, F));
        const float* vertices = static_cast<const float*>(vertices_f32_dev);
        const u32* faces = static_cast<const u32*>(faces_u32_dev);
        const u32* colours = static_cast<const u32*>(colours_rgba8_dev);
        WDGS_CHECK_HIP(hipMemsetAsync(s->totals, 0, sizeof(u32) * MS_T_WORDS, d->stream));
        WDGS_TRY(launch_simplify_cell_keys(d, vertices, V, origin, inv, cell_size, s->vertex_keys));
        WDGS_TRY(s->sort.rank(d, s->vertex_keys, V, s->totals + MS_T_DISTINCT, s->rank, s->cluster_keys, nullptr, nullptr, nullptr, nullptr));
        WDGS_TRY(launch_simplify_accumulate(d, vertices, colours, s->rank, V, origin, inv, cell_size, s->acc));
        WDGS_TRY(launch_simplify_finalize(d, s->cluster_keys, s->totals, s->acc, V, origin, inv, cell_size, colours != nullptr, s->cluster_positions, s->cluster_colours));
        if (F != 0u) WDGS_TRY(launch_simplify_face_keys(d, faces, F, V, s->vertex_keys, s->rank, s->face_keys, s->lead, s->iota, s->partial));
        WDGS_TRY(launch_simplify_fold(d, s->partial, simplify_partial_rows(F), s->cluster_keys, s->totals));
        if (F != 0u) {
            WDGS_TRY(s->sort.rank(d, s->face_keys, F, s->totals + MS_T_SPARE, s->face_rank, nullptr, nullptr, nullptr, nullptr, nullptr));
            WDGS_TRY(launch_simplify_face_keys2(d, s->lead, s->face_rank, F, s->face_keys));
            WDGS_TRY(s->sort.rank(d, s->face_keys, F, s->totals + MS_T_SPARE, s->face_rank, nullptr, s->iota, s->head_face, nullptr, nullptr));   // (lowest face per key)
            WDGS_TRY(launch_simplify_mark(d, faces, F, V, s->lead, s->face_rank, s->head_face, s->rank, s->face_flags, s->cluster_flags));
            WDGS_TRY(scan_exclusive_u32(d, s->sort.scan(), s->cluster_flags, s->cluster_offsets, V, s->totals + MS_T_VERTICES));
            WDGS_TRY(scan_exclusive_u32(d, s->sort.scan(), s->face_flags, s->face_offsets, F, s->totals + MS_T_FACES));
        } else {
            WDGS_CHECK_HIP(hipMemsetAsync(s->cluster_flags, 0, sizeof(u32) * (size_t)V, d->stream));
        }
        WDGS_CHECK_HIP(hipMemcpyAsync(host, s->totals, sizeof(host), hipMemcpyDeviceToHost, d->stream));
        WDGS_CHECK_HIP(wdgs_sync_lanes(d));
    }
    s->vertices = vertices_f32_dev;
    s->faces = faces_u32_dev;
    s->colours = colours_rgba8_dev;
    s->V = V;
    s->F = F;
    s->clusters = host[MS_T_DISTINCT] - host[MS_T_HAS_OUTSIDE];
    s->vertices_out = host[MS_T_VERTICES];
    s->faces_out = host[MS_T_FACES];
    s->invalid = host[MS_T_INVALID];
    s->outside = host[MS_T_OUTSIDE];
    s->collapsed = host[MS_T_COLLAPSED];
    s->duplicate = F - s->invalid - s->outside - s->collapsed - s->faces_out;
    s->counted = true;
    *vertices_out = s->vertices_out;
    *faces_out = s->faces_out;
    return WDGS_OK;
}

extern "C" int wdgs_mesh_simplifier_emit(wdgs_mesh_simplifier* s, const void* vertices_f32_dev, uint32_t num_vertices, const void* faces_u32_dev, uint32_t num_faces,
                                         const void* colours_rgba8_dev, void* vertices_out_f32_dev, void* colours_out_rgba8_dev, void* keys_out_u64_dev,
                                         void* faces_out_u32_dev, void* face_map_u32_dev, void* vertex_cluster_u32_dev, uint32_t capacity_vertices, uint32_t capacity_faces) {
    WDGS_REQUIRE(s, WDGS_E_INVALID, "wdgs_mesh_simplifier_emit: null argument");
    WDGS_REQUIRE(s->counted && vertices_f32_dev == s->vertices && faces_u32_dev == s->faces && colours_rgba8_dev == s->colours && num_vertices == s->V && num_faces == s->F,
                 WDGS_E_STATE, "simplifyMesh: no count of this mesh precedes the emit");
    WDGS_REQUIRE(capacity_vertices >= s->vertices_out && capacity_faces >= s->faces_out, WDGS_E_CAPACITY, "simplifyMesh: %u vertices and %u faces, room for %u and %u",
                 s->vertices_out, s->faces_out, capacity_vertices, capacity_faces);
    WDGS_REQUIRE((colours_rgba8_dev == nullptr) == (colours_out_rgba8_dev == nullptr), WDGS_E_INVALID, "wdgs_mesh_simplifier_emit: colours need both an input and an output");
    WDGS_REQUIRE((s->vertices_out == 0 || vertices_out_f32_dev) && (s->faces_out == 0 || faces_out_u32_dev), WDGS_E_INVALID,
                 "wdgs_mesh_simplifier_emit: null vertices or faces output");
    WDGS_REQUIRE((((uintptr_t)vertices_out_f32_dev | (uintptr_t)colours_out_rgba8_dev | (uintptr_t)faces_out_u32_dev | (uintptr_t)face_map_u32_dev |
                   (uintptr_t)vertex_cluster_u32_dev) & 3u) == 0u && ((uintptr_t)keys_out_u64_dev & 7u) == 0u,
                 WDGS_E_INVALID, "wdgs_mesh_simplifier_emit: misaligned buffer");
    if (s->V == 0) return WDGS_OK;
    return launch_simplify_emit(s->dev, static_cast<const u32*>(faces_u32_dev), s->F, s->V, s->totals, s->cluster_flags, s->cluster_offsets, s->cluster_keys,
                                s->cluster_positions, s->cluster_colours, s->vertex_keys, s->rank, s->face_flags, s->face_offsets, static_cast<float*>(vertices_out_f32_dev),
                                static_cast<u32*>(colours_out_rgba8_dev), static_cast<unsigned long long*>(keys_out_u64_dev), static_cast<u32*>(faces_out_u32_dev),
                                static_cast<u32*>(face_map_u32_dev), static_cast<u32*>(vertex_cluster_u32_dev));
}

extern "C" int wdgs_mesh_simplifier_stats(const wdgs_mesh_simplifier* s, uint32_t* clusters, uint32_t* invalid_faces, uint32_t* outside_faces, uint32_t* collapsed_faces,
                                          uint32_t* duplicate_faces, uint32_t* vertices_out, uint32_t* faces_out) {
    WDGS_REQUIRE(s, WDGS_E_INVALID, "wdgs_mesh_simplifier_stats: null argument");
    WDGS_REQUIRE(s->counted, WDGS_E_STATE, "simplifyMesh: no count precedes the read of its statistics");
    if (clusters) *clusters = s->clusters;
    if (invalid_faces) *invalid_faces = s->invalid;
    if (outside_faces) *outside_faces = s->outside;
    if (collapsed_faces) *collapsed_faces = s->collapsed;
    if (duplicate_faces) *duplicate_faces = s->duplicate;
    if (vertices_out) *vertices_out = s->vertices_out;
    if (faces_out) *faces_out = s->faces_out;
    return WDGS_OK;
}
