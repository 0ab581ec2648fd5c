// A z-buffered triangle rasterizer under the library's camera block, and the agreement of two depth images (no counterpart in the
// reference, which renders splats only).  include/webdgs.h states the definition operation by operation; tests/meshraster_ref.py restates it.
//
// Coverage is decided in 64-bit integers on positions snapped to 1/256 pixel; depth is four f32 divisions per fragment in a fixed order; the hidden-surface
// test is ONE unsigned 64-bit atomic min of (bits(depth) << 32 | face) per fragment into a u64 image cleared to all ones.  A minimum does not depend on the
// order of its operands, so the image is a function of the input alone whatever the order of faces, waves or launches.  The statistics are integer adds.
//
// Five launches and the library's scan, in this order:
//   raster_vertices   one thread per vertex: the view-space position and the fixed-point screen position (20 bytes per vertex)
//   raster_faces      one thread per face: its class; a SMALL face (bounding box at most WDGS_MESH_RASTER_LARGE_FACE_PIXELS on both axes) is rasterized here,
//                     its three edge functions advanced by additions; a LARGE face leaves counts[f] = the 8 x 8 pixel blocks of its bounding box
//   scan              offsets = the exclusive scan of counts, and its total: the number of (face, block) work items
//   raster_blocks     a fixed grid whose waves share the items out in contiguous runs, one lane per pixel; item -> face by a binary search of offsets, so that
//                     no item array of a size only the device knows has to be allocated and the host never waits
//   raster_resolve    one thread per pixel: the outputs asked for
// Section 16's to 19's rule holds: no spin-wait, no inter-workgroup flag, no look-back, no grid barrier, no float atomics; visibility comes from launch
// boundaries only; the integer atomics (the z-buffer's min, the statistics' adds) go to words that no kernel of the same launch reads except for the early-out
// below, which is exact for any value it may see.
#include <algorithm>
#include <cmath>
#include <memory>

#include "dmath.h"
#include "launch.h"

namespace {

typedef unsigned long long u64;
typedef long long i64;

constexpr u32 MR_THREADS = 256;
constexpr u32 MR_WAVES = MR_THREADS / 64;
constexpr u32 MR_VERTEX_WORDS = 5;            // X, Y (i32) and the view-space position (f32 x 3)
constexpr i32 MR_UNUSABLE = (i32)0x80000000;  // X of a vertex that is not usable (a usable |X| is at most 2^22)
constexpr u32 MR_BLOCKS_WG_PER_CU = 8;        // raster_blocks' fixed grid
constexpr u32 MR_NO_FACE = 0xFFFFFFFFu;
constexpr u64 MR_EMPTY = ~0ull;
// The statistics block, u32 words: the six face classes in the order of the definition, the covered pixels, the viewport flag; then the work items as the
// u64 sum of counts (words 8, 9) and as the scan's u32 total
constexpr u32 MR_S_INVALID = 0, MR_S_CLIPPED = 1, MR_S_DEGENERATE = 2, MR_S_CULLED = 3, MR_S_EMPTY = 4, MR_S_RASTERIZED = 5, MR_S_COVERED = 6, MR_S_MISMATCH = 7,
              MR_S_ITEMS64 = 8, MR_S_ITEMS = 10, MR_S_WORDS = 12;
constexpr u32 MR_CLASSES = 6;

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) < __builtin_inff(); }

__device__ __forceinline__ u32 wave_sum(u32 x) {
#pragma unroll
    for (u32 d = 32; d >= 1; d >>= 1) x += (u32)__shfl_xor((int)x, (int)d, 64);
    return x;
}

__device__ __forceinline__ bool viewport_matches(const float* __restrict__ camera, u32 W, u32 H) { return camera[64] == (float)W && camera[65] == (float)H; }

// ---- the vertex: wdgs_tsdf_volume_integrate's arithmetic (tsdf.hip), then the snap to 1/256 pixel
__global__ __launch_bounds__(MR_THREADS) void mr_vertices_kernel(const float* __restrict__ vertices, u32 V, const float* __restrict__ camera, u32 W, u32 H, float near,
                                                                 u32* __restrict__ records) {
    const u32 v = blockIdx.x * MR_THREADS + threadIdx.x;
    if (v >= V) return;
    const float px = vertices[3u * (size_t)v], py = vertices[3u * (size_t)v + 1u], pz = vertices[3u * (size_t)v + 2u];
    const float vx = ((camera[0] * px + camera[4] * py) + camera[8] * pz) + camera[12];
    const float vy = ((camera[1] * px + camera[5] * py) + camera[9] * pz) + camera[13];
    const float z = ((camera[2] * px + camera[6] * py) + camera[10] * pz) + camera[14];
    const float sx = (wd_div(camera[32] * vx, z) * 0.5f + 0.5f) * (float)W;
    const float sy = (wd_div((-camera[37]) * vy, z) * 0.5f + 0.5f) * (float)H;
    const bool usable = finite_f(vx) && finite_f(vy) && finite_f(z) && z >= near && finite_f(sx) && finite_f(sy) && fabsf(sx) <= 16384.0f && fabsf(sy) <= 16384.0f;
    u32* r = records + MR_VERTEX_WORDS * (size_t)v;
    r[0] = usable ? (u32)(i32)__builtin_rintf(sx * 256.0f) : (u32)MR_UNUSABLE;
    r[1] = usable ? (u32)(i32)__builtin_rintf(sy * 256.0f) : 0u;
    r[2] = __float_as_uint(vx);
    r[3] = __float_as_uint(vy);
    r[4] = __float_as_uint(z);
}

// ---- the face: what both rasterizing kernels and the resolve derive from its three records
struct MrCorners {
    i32 X[3], Y[3];
    float w[3];   // 1 / z
    i64 A;
};

__device__ __forceinline__ bool load_corners(const u32* __restrict__ records, const u32 c[3], MrCorners& t) {
    bool usable = true;
#pragma unroll
    for (u32 k = 0; k < 3u; k++) {
        const u32* r = records + MR_VERTEX_WORDS * (size_t)c[k];
        t.X[k] = (i32)r[0];
        t.Y[k] = (i32)r[1];
        t.w[k] = wd_div(1.0f, __uint_as_float(r[4]));
        usable = usable && t.X[k] != MR_UNUSABLE;
    }
    t.A = (i64)(t.X[1] - t.X[0]) * (i64)(t.Y[2] - t.Y[0]) - (i64)(t.X[2] - t.X[0]) * (i64)(t.Y[1] - t.Y[0]);
    return usable;
}

// The three edge functions at the centre of pixel (i, j), their steps per pixel along x and y, and what a covered pixel's value is at least: 0 on an edge that
// owns its line, 1 on one that does not
struct MrEdges {
    i64 e[3], dx[3], dy[3], least[3];
};

__device__ __forceinline__ MrEdges edges_at(const MrCorners& t, i32 i, i32 j) {
    MrEdges g;
    const i64 s = t.A > 0 ? 1 : -1;
    const i64 cx = 256 * (i64)i + 128, cy = 256 * (i64)j + 128;
#pragma unroll
    for (u32 k = 0; k < 3u; k++) {
        const u32 a = (k + 1u) % 3u, b = (k + 2u) % 3u;
        const i64 ex = (i64)t.X[b] - t.X[a], ey = (i64)t.Y[b] - t.Y[a];
        g.e[k] = s * (ex * (cy - t.Y[a]) - ey * (cx - t.X[a]));
        const i64 alpha = -s * ey, beta = s * ex;
        g.dx[k] = 256 * alpha;
        g.dy[k] = 256 * beta;
        g.least[k] = (alpha > 0 || (alpha == 0 && beta > 0)) ? 0 : 1;
    }
    return g;
}

__device__ __forceinline__ bool covered(const i64 e[3], const MrEdges& g) { return e[0] >= g.least[0] && e[1] >= g.least[1] && e[2] >= g.least[2]; }

// lambda_k = f32(e_k) / f32(|A|) and the perspective-correct depth 1 / ((l0 w0 + l1 w1) + l2 w2)
__device__ __forceinline__ float fragment_depth(const i64 e[3], float area, const float w[3], float lw[3]) {
#pragma unroll
    for (u32 k = 0; k < 3u; k++) lw[k] = wd_div((float)e[k], area) * w[k];
    return wd_div(1.0f, (lw[0] + lw[1]) + lw[2]);
}

// One fragment: a relaxed load first -- the words only ever decrease, so a fragment that is not below what the load saw is not below what is there
__device__ __forceinline__ void depth_test(u64* __restrict__ zbuf, size_t p, const i64 e[3], float area, const float w[3], u32 f) {
    float lw[3];
    const float zp = fragment_depth(e, area, w, lw);
    if (!(zp > 0.0f && zp < __builtin_inff())) return;
    const u64 word = ((u64)__float_as_uint(zp) << 32) | f;
    if (word < __hip_atomic_load(zbuf + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(zbuf + p, word);
}

// The pixels of the viewport whose centres lie in the face's bounding box: [lo, hi] per axis, empty when lo > hi
struct MrBox { i32 i_lo, i_hi, j_lo, j_hi; };
__device__ __forceinline__ MrBox pixel_box(const MrCorners& t, u32 W, u32 H) {
    const i32 x_min = min(t.X[0], min(t.X[1], t.X[2])), x_max = max(t.X[0], max(t.X[1], t.X[2]));
    const i32 y_min = min(t.Y[0], min(t.Y[1], t.Y[2])), y_max = max(t.Y[0], max(t.Y[1], t.Y[2]));
    MrBox b;
    b.i_lo = max((x_min + 127) >> 8, 0);   // the first i with 256 i + 128 >= x_min
    b.i_hi = min((x_max - 128) >> 8, (i32)W - 1);
    b.j_lo = max((y_min + 127) >> 8, 0);
    b.j_hi = min((y_max - 128) >> 8, (i32)H - 1);
    return b;
}
__device__ __forceinline__ bool is_large(const MrBox& b) {
    return b.i_hi - b.i_lo >= (i32)WDGS_MESH_RASTER_LARGE_FACE_PIXELS || b.j_hi - b.j_lo >= (i32)WDGS_MESH_RASTER_LARGE_FACE_PIXELS;
}
__device__ __forceinline__ u32 block_columns(const MrBox& b) { return (u32)((b.i_hi >> 3) - (b.i_lo >> 3) + 1); }
__device__ __forceinline__ u32 block_rows(const MrBox& b) { return (u32)((b.j_hi >> 3) - (b.j_lo >> 3) + 1); }

// One thread per face.  counts[f]: the work items a large face leaves for raster_blocks, 0 for every other face
__global__ __launch_bounds__(MR_THREADS) void mr_faces_kernel(const u32* __restrict__ faces, u32 F, u32 V, const u32* __restrict__ records, const float* __restrict__ camera,
                                                              u32 W, u32 H, u32 cull, u64* __restrict__ zbuf, u32* __restrict__ counts, u32* __restrict__ stats) {
    __shared__ u32 s_class[MR_CLASSES];
    __shared__ u32 s_items;
    if (threadIdx.x < MR_CLASSES) s_class[threadIdx.x] = 0u;
    if (threadIdx.x == MR_CLASSES) s_items = 0u;
    __syncthreads();
    const u32 f = blockIdx.x * MR_THREADS + threadIdx.x;
    u32 cls = MR_CLASSES, items = 0u;
    if (f < F) {
        u32 c[3];
#pragma unroll
        for (u32 k = 0; k < 3u; k++) c[k] = faces[3u * (size_t)f + k];
        MrCorners t;
        if (c[0] >= V || c[1] >= V || c[2] >= V) cls = MR_S_INVALID;
        else if (!load_corners(records, c, t)) cls = MR_S_CLIPPED;
        else if (t.A == 0) cls = MR_S_DEGENERATE;
        else if ((cull == WDGS_CULL_BACK && t.A > 0) || (cull == WDGS_CULL_FRONT && t.A < 0)) cls = MR_S_CULLED;   // (front: A < 0; the header derives it)
        else {
            const MrBox b = pixel_box(t, W, H);
            if (b.i_lo > b.i_hi || b.j_lo > b.j_hi) cls = MR_S_EMPTY;
            else {
                cls = MR_S_RASTERIZED;
                if (!viewport_matches(camera, W, H)) {
                    // (a camera block of another image size: classified, never drawn)
                } else if (is_large(b)) {
                    items = block_columns(b) * block_rows(b);
                } else {
                    const MrEdges g = edges_at(t, b.i_lo, b.j_lo);
                    const float area = (float)(t.A > 0 ? t.A : -t.A);
                    i64 row[3] = {g.e[0], g.e[1], g.e[2]};
                    for (i32 j = b.j_lo; j <= b.j_hi; j++) {
                        i64 e[3] = {row[0], row[1], row[2]};
                        for (i32 i = b.i_lo; i <= b.i_hi; i++) {
                            if (covered(e, g)) depth_test(zbuf, (size_t)j * W + (u32)i, e, area, t.w, f);
#pragma unroll
                            for (u32 k = 0; k < 3u; k++) e[k] += g.dx[k];
                        }
#pragma unroll
                        for (u32 k = 0; k < 3u; k++) row[k] += g.dy[k];
                    }
                }
            }
        }
        counts[f] = items;
    }
    if (cls < MR_CLASSES) atomicAdd(&s_class[cls], 1u);
    if (items != 0u) atomicAdd(&s_items, items);   // (at most 256 faces of at most 2^20 blocks each)
    __syncthreads();
    if (threadIdx.x < MR_CLASSES && s_class[threadIdx.x] != 0u) atomicAdd(stats + threadIdx.x, s_class[threadIdx.x]);
    if (threadIdx.x == MR_CLASSES && s_items != 0u) atomicAdd(reinterpret_cast<u64*>(stats + MR_S_ITEMS64), (u64)s_items);
}

// Work item `local` of large face f, whose corners and box are t and b, by one wave: block (local % columns, local / columns) of the face's block grid, lane l
// the pixel (l % 8, l / 8) of it
__device__ __forceinline__ void raster_block(const MrCorners& t, const MrBox& b, u32 f, u32 local, u32 W, u64* __restrict__ zbuf) {
    const u32 columns = block_columns(b);
    const i32 i0 = (i32)(((u32)(b.i_lo >> 3) + local % columns) << 3), j0 = (i32)(((u32)(b.j_lo >> 3) + local / columns) << 3);
    MrEdges g = edges_at(t, i0, j0);
    // a block that lies wholly outside an edge: the edge function is linear, so its largest value over the block's pixel centres is at a corner
#pragma unroll
    for (u32 k = 0; k < 3u; k++) {
        const i64 most = g.e[k] + (g.dx[k] > 0 ? 7 * g.dx[k] : 0) + (g.dy[k] > 0 ? 7 * g.dy[k] : 0);
        if (most < g.least[k]) return;
    }
    const i32 li = (i32)(threadIdx.x & 7u), lj = (i32)((threadIdx.x >> 3) & 7u);
    const i32 i = i0 + li, j = j0 + lj;
    if (i < b.i_lo || i > b.i_hi || j < b.j_lo || j > b.j_hi) return;
    i64 e[3];
#pragma unroll
    for (u32 k = 0; k < 3u; k++) e[k] = g.e[k] + li * g.dx[k] + lj * g.dy[k];
    if (covered(e, g)) depth_test(zbuf, (size_t)j * W + (u32)i, e, (float)(t.A > 0 ? t.A : -t.A), t.w, f);
}

__device__ __forceinline__ MrBox load_large_face(const u32* __restrict__ faces, u32 f, const u32* __restrict__ records, u32 W, u32 H, MrCorners& t) {
    u32 c[3];
#pragma unroll
    for (u32 k = 0; k < 3u; k++) c[k] = faces[3u * (size_t)f + k];
    (void)load_corners(records, c, t);   // (counts[f] != 0: the face is valid, usable and of non-zero area)
    return pixel_box(t, W, H);
}

// A fixed grid.  The work items, whose number every wave reads from the statistics block, are dealt to the waves in equal contiguous runs, so that a wave finds
// its face -- a binary search of the offsets, three dependent loads and the set-up -- once per face of its run and not once per item (a hundred faces that fill
// 1920 x 1080 are 3.2 M items: found item by item, the searches' latency was the whole of the kernel's time).  Should the items number 2^32 or more (the u64 sum
// says so; the scan's offsets have then wrapped) the waves stride over the faces instead and take each large face's blocks in turn.
__global__ __launch_bounds__(MR_THREADS) void mr_blocks_kernel(const u32* __restrict__ faces, u32 F, const u32* __restrict__ records, u32 W, u32 H,
                                                               const u32* __restrict__ counts, const u32* __restrict__ offsets, const u32* __restrict__ stats,
                                                               u64* __restrict__ zbuf) {
    const u32 wave = (u32)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * MR_WAVES + (threadIdx.x >> 6)));
    const u32 waves = gridDim.x * MR_WAVES;
    const u64 items = *reinterpret_cast<const u64*>(stats + MR_S_ITEMS64);
    MrCorners t;
    if (items <= 0xFFFFFFFFull) {
        const u64 run = (items + waves - 1u) / waves;
        const u64 end = min(items, (wave + 1ull) * run);
        u32 f = 0u, first = 0u, last = 0u;   // the face whose items are [first, last): none yet
        MrBox b = {0, 0, 0, 0};
        for (u64 item = wave * run; item < end; item++) {
            if ((u32)item >= last) {
                u32 lo = 0u, hi = F;   // the last face whose offset is <= item: it alone has the item among its counts
                while (lo < hi) {
                    const u32 mid = lo + (hi - lo) / 2u;
                    if (offsets[mid] <= (u32)item) lo = mid + 1u; else hi = mid;
                }
                f = lo - 1u;
                first = offsets[f];
                last = first + counts[f];
                b = load_large_face(faces, f, records, W, H, t);
            }
            raster_block(t, b, f, (u32)item - first, W, zbuf);
        }
    } else {
        for (u64 f = wave; f < (u64)F; f += waves) {
            const u32 n = counts[f];
            if (n == 0u) continue;
            const MrBox b = load_large_face(faces, (u32)f, records, W, H, t);
            for (u32 local = 0u; local < n; local++) raster_block(t, b, (u32)f, local, W, zbuf);
        }
    }
}

// One thread per pixel: the outputs asked for (each nullable), the covered pixels and the viewport flag
__global__ __launch_bounds__(MR_THREADS) void mr_resolve_kernel(const u64* __restrict__ zbuf, u32 W, u32 H, const u32* __restrict__ faces, u32 V,
                                                                const u32* __restrict__ records, const u32* __restrict__ colours, const float* __restrict__ camera,
                                                                float* __restrict__ depth_out, u32* __restrict__ face_out, u32* __restrict__ colour_out,
                                                                float4* __restrict__ normal_out, u32* __restrict__ stats) {
    __shared__ u32 s_covered[MR_WAVES];
    const u32 p = blockIdx.x * MR_THREADS + threadIdx.x;
    u32 hit = 0u;
    if (p < W * H) {
        const u64 word = zbuf[p];
        float depth = 0.0f;
        u32 f = MR_NO_FACE, colour = 0u;
        float4 normal = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (word != MR_EMPTY) {
            hit = 1u;
            f = (u32)word;
            depth = __uint_as_float((u32)(word >> 32));
            if (colour_out || normal_out) {
                u32 c[3];
#pragma unroll
                for (u32 k = 0; k < 3u; k++) c[k] = min(faces[3u * (size_t)f + k], V - 1u);   // (a drawn face's indices are < V)
                if (colour_out) {
                    MrCorners t;
                    (void)load_corners(records, c, t);
                    const MrEdges g = edges_at(t, (i32)(p % W), (i32)(p / W));
                    float lw[3];
                    const float zp = fragment_depth(g.e, (float)(t.A > 0 ? t.A : -t.A), t.w, lw);   // (the bits of `depth`: the same operations)
                    const u32 c0 = colours[c[0]], c1 = colours[c[1]], c2 = colours[c[2]];
                    colour = 0xFF000000u;
#pragma unroll
                    for (u32 ch = 0; ch < 3u; ch++) {
                        const float C0 = (float)((c0 >> (8u * ch)) & 0xFFu), C1 = (float)((c1 >> (8u * ch)) & 0xFFu), C2 = (float)((c2 >> (8u * ch)) & 0xFFu);
                        const float tsum = (lw[0] * C0 + lw[1] * C1) + lw[2] * C2;
                        colour |= (u32)__builtin_rintf(wd_min(wd_max(tsum * zp, 0.0f), 255.0f)) << (8u * ch);
                    }
                }
                if (normal_out) {
                    float v[3][3];
#pragma unroll
                    for (u32 k = 0; k < 3u; k++) {
#pragma unroll
                        for (u32 a = 0; a < 3u; a++) v[k][a] = __uint_as_float(records[MR_VERTEX_WORDS * (size_t)c[k] + 2u + a]);
                    }
                    const float ax = v[1][0] - v[0][0], ay = v[1][1] - v[0][1], az = v[1][2] - v[0][2];
                    const float bx = v[2][0] - v[0][0], by = v[2][1] - v[0][1], bz = v[2][2] - v[0][2];
                    const float gx = ay * bz - az * by, gy = az * bx - ax * bz, gz = ax * by - ay * bx;
                    const float len = wd_sqrt((gx * gx + gy * gy) + gz * gz);
                    float nx = wd_div(gx, len), ny = wd_div(gy, len), nz = wd_div(gz, len);
                    if ((nx * v[0][0] + ny * v[0][1]) + nz * v[0][2] > 0.0f) { nx = -nx; ny = -ny; nz = -nz; }
                    const bool zero = nx == 0.0f && ny == 0.0f && nz == 0.0f;
                    if (finite_f(nx) && finite_f(ny) && finite_f(nz) && !zero) normal = make_float4(nx, ny, nz, 1.0f);
                }
            }
        }
        if (depth_out) depth_out[p] = depth;
        if (face_out) face_out[p] = f;
        if (colour_out) colour_out[p] = colour;
        if (normal_out) normal_out[p] = normal;
    }
    hit = wave_sum(hit);
    if ((threadIdx.x & 63u) == 0u) s_covered[threadIdx.x >> 6] = hit;
    __syncthreads();
    if (threadIdx.x == 0u) {
        const u32 n = (s_covered[0] + s_covered[1]) + (s_covered[2] + s_covered[3]);
        if (n != 0u) atomicAdd(stats + MR_S_COVERED, n);
        if (blockIdx.x == 0u) stats[MR_S_MISMATCH] = viewport_matches(camera, W, H) ? 0u : 1u;
    }
}

// ---- the agreement of two depth images: five exact integer sums (geometry.hip's distance_stats_kernel is the model)
__device__ __forceinline__ bool depth_present(float d) { return d > 0.0f && d < __builtin_inff(); }

__global__ __launch_bounds__(MR_THREADS) void depth_agreement_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ b_weight_sum,
                                                                     float min_weight_sum, u32 npix, float max_difference, float threshold, u64* __restrict__ out) {
    __shared__ u64 s_w[5][MR_WAVES];
    u64 acc[5] = {0ull, 0ull, 0ull, 0ull, 0ull};   // both, onlyA, onlyB, within, sum_q
    for (u32 p = blockIdx.x * MR_THREADS + threadIdx.x; p < npix; p += gridDim.x * MR_THREADS) {
        const float da = a[p], db = b[p];
        const bool has_a = depth_present(da), has_b = depth_present(db) && (!b_weight_sum || b_weight_sum[p] >= min_weight_sum);
        if (has_a && has_b) {
            const float d = fabsf(da - db);
            acc[0] += 1ull;
            if (d <= threshold) acc[3] += 1ull;
            acc[4] += (u64)wd_to_u32(wd_min(wd_div(d, max_difference), 1.0f) * 16777216.0f);
        } else if (has_a) {
            acc[1] += 1ull;
        } else if (has_b) {
            acc[2] += 1ull;
        }
    }
#pragma unroll
    for (u32 k = 0; k < 5u; k++) {
#pragma unroll
        for (u32 d = 32; d >= 1; d >>= 1) acc[k] += (u64)__shfl_xor((i64)acc[k], (int)d, 64);
        if ((threadIdx.x & 63u) == 0u) s_w[k][threadIdx.x >> 6] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < 5u) {
        const u64 s = (s_w[threadIdx.x][0] + s_w[threadIdx.x][1]) + (s_w[threadIdx.x][2] + s_w[threadIdx.x][3]);
        if (s) atomicAdd(out + threadIdx.x, s);
    }
}

bool positive_finite(float x) { return x > 0.0f && x < __builtin_inff(); }

}  // namespace

// ---------------------------------------------------------------- the C ABI object (include/webdgs.h)
struct wdgs_mesh_rasterizer {
    wdgs_device* dev = nullptr;
    DevMem<u32> records;           // [5 V]
    DevMem<u64> zbuf;              // [W H]
    DevMem<u32> counts, offsets;   // [F]: the large faces' work items and their exclusive scan
    ScanScratch scan;
    DevMem<u32> stats;             // MR_S_WORDS
    size_t capacity_v = 0, capacity_f = 0, capacity_px = 0;
    bool encoded = false;
};

extern "C" int wdgs_mesh_rasterizer_create(wdgs_device* dev, wdgs_mesh_rasterizer** out) {
    WDGS_REQUIRE(dev && out, WDGS_E_INVALID, "wdgs_mesh_rasterizer_create: null argument");
    WDGS_REQUIRE(!dev->capturing, WDGS_E_STATE, "wdgs_mesh_rasterizer_create while recording a command buffer");
    auto r = std::make_unique<wdgs_mesh_rasterizer>();
    r->dev = dev;
    WDGS_TRY(r->stats.alloc(MR_S_WORDS, true, dev->stream));
    *out = r.release();
    return WDGS_OK;
}

extern "C" int wdgs_mesh_rasterizer_destroy(wdgs_mesh_rasterizer* r) {
    if (!r) return WDGS_OK;
    if (wdgs_device_alive(r->dev) && !r->dev->capturing) (void)wdgs_sync_lanes(r->dev);
    delete r;
    return WDGS_OK;
}

extern "C" int wdgs_mesh_rasterizer_encode(wdgs_mesh_rasterizer* r, const void* vertices_f32_dev, uint32_t num_vertices, const void* faces_u32_dev, uint32_t num_faces,
                                           const void* colours_rgba8_dev, const void* camera_dev, uint32_t width, uint32_t height, float near, uint32_t cull,
                                           void* depth_out_f32_dev, void* face_out_u32_dev, void* colour_out_rgba8_dev, void* normal_out_rgba32f_dev) {
    WDGS_REQUIRE(r && camera_dev, WDGS_E_INVALID, "wdgs_mesh_rasterizer_encode: null argument");
    WDGS_REQUIRE(num_vertices < (1u << 31) && 3ull * num_faces < (1ull << 32), WDGS_E_INVALID, "rasterizeMesh: %u vertices and %u faces: 2^31 vertices or 2^32 face indices or more",
                 num_vertices, num_faces);
    WDGS_REQUIRE(width >= 1u && width <= WDGS_MESH_RASTER_MAX_SIZE && height >= 1u && height <= WDGS_MESH_RASTER_MAX_SIZE, WDGS_E_INVALID,
                 "rasterizeMesh: bad image size %ux%u (1 to %u)", width, height, WDGS_MESH_RASTER_MAX_SIZE);
    WDGS_REQUIRE(positive_finite(near), WDGS_E_INVALID, "rasterizeMesh: near %g must be positive and finite", (double)near);
    WDGS_REQUIRE(cull <= WDGS_CULL_FRONT, WDGS_E_INVALID, "rasterizeMesh: unknown cull mode %u", cull);
    WDGS_REQUIRE((num_vertices == 0 || vertices_f32_dev) && (num_faces == 0 || faces_u32_dev), WDGS_E_INVALID, "wdgs_mesh_rasterizer_encode: null vertices or faces");
    WDGS_REQUIRE(!colour_out_rgba8_dev || colours_rgba8_dev, WDGS_E_INVALID, "rasterizeMesh: a colour image needs vertex colours");
    WDGS_REQUIRE((((uintptr_t)vertices_f32_dev | (uintptr_t)faces_u32_dev | (uintptr_t)colours_rgba8_dev | (uintptr_t)camera_dev | (uintptr_t)depth_out_f32_dev |
                   (uintptr_t)face_out_u32_dev | (uintptr_t)colour_out_rgba8_dev) & 3u) == 0u && ((uintptr_t)normal_out_rgba32f_dev & 15u) == 0u,
                 WDGS_E_INVALID, "wdgs_mesh_rasterizer_encode: misaligned buffer (4 bytes; the normal image 16)");
    wdgs_device* d = r->dev;
    const u32 V = num_vertices, F = num_faces, W = width, H = height;
    const size_t npix = (size_t)W * H;
    if (V > r->capacity_v || F > r->capacity_f || npix > r->capacity_px) {
        WDGS_REQUIRE(!d->capturing, WDGS_E_STATE, "rasterizeMesh: the object's arrays have to grow, which cannot be recorded into a command buffer (encode once before recording)");
        WDGS_CHECK_HIP(wdgs_sync_lanes(d));   // (nothing in flight may still read the blocks given back)
        if (V > r->capacity_v) {
            r->capacity_v = 0;
            WDGS_TRY(r->records.alloc((size_t)MR_VERTEX_WORDS * V, false, d->stream));
            r->capacity_v = V;
        }
        if (F > r->capacity_f) {
            r->capacity_f = 0;
            WDGS_TRY(r->counts.alloc(F, false, d->stream));
            WDGS_TRY(r->offsets.alloc(F, false, d->stream));
            WDGS_TRY(scan_scratch_create(&r->scan, F));
            r->capacity_f = F;
        }
        if (npix > r->capacity_px) {
            r->capacity_px = 0;
            WDGS_TRY(r->zbuf.alloc(npix, false, d->stream));
            r->capacity_px = npix;
        }
    }
    const float* camera = static_cast<const float*>(camera_dev);
    const u32* faces = static_cast<const u32*>(faces_u32_dev);
    WDGS_CHECK_HIP(hipMemsetAsync(r->stats, 0, sizeof(u32) * MR_S_WORDS, d->stream));
    WDGS_CHECK_HIP(hipMemsetAsync(r->zbuf, 0xFF, sizeof(u64) * npix, d->stream));
    if (V != 0u)
        WDGS_LAUNCH(d, "raster_vertices", mr_vertices_kernel, dim3(ceil_div(V, MR_THREADS)), dim3(MR_THREADS), 0, static_cast<const float*>(vertices_f32_dev), V, camera, W, H,
                    near, r->records.get());
    if (F != 0u) {
        WDGS_LAUNCH(d, "raster_faces", mr_faces_kernel, dim3(ceil_div(F, MR_THREADS)), dim3(MR_THREADS), 0, faces, F, V, (const u32*)r->records, camera, W, H, cull,
                    r->zbuf.get(), r->counts.get(), r->stats.get());
        WDGS_CHECK_HIP(hipGetLastError());
        WDGS_TRY(scan_exclusive_u32(d, &r->scan, r->counts, r->offsets, F, r->stats + MR_S_ITEMS));
        WDGS_LAUNCH(d, "raster_blocks", mr_blocks_kernel, dim3((u32)d->num_cus * MR_BLOCKS_WG_PER_CU), dim3(MR_THREADS), 0, faces, F, (const u32*)r->records, W, H,
                    (const u32*)r->counts, (const u32*)r->offsets, (const u32*)r->stats, r->zbuf.get());
    }
    WDGS_LAUNCH(d, "raster_resolve", mr_resolve_kernel, dim3((u32)((npix + MR_THREADS - 1u) / MR_THREADS)), dim3(MR_THREADS), 0, (const u64*)r->zbuf, W, H, faces, V,
                (const u32*)r->records, static_cast<const u32*>(colours_rgba8_dev), camera, static_cast<float*>(depth_out_f32_dev), static_cast<u32*>(face_out_u32_dev),
                static_cast<u32*>(colour_out_rgba8_dev), static_cast<float4*>(normal_out_rgba32f_dev), r->stats.get());
    WDGS_CHECK_HIP(hipGetLastError());
    r->encoded = true;
    return WDGS_OK;
}

extern "C" int wdgs_mesh_rasterizer_stats(wdgs_mesh_rasterizer* r, uint32_t* invalid_faces, uint32_t* clipped_faces, uint32_t* degenerate_faces, uint32_t* culled_faces,
                                          uint32_t* empty_faces, uint32_t* rasterized_faces, uint32_t* covered_pixels, uint32_t* viewport_mismatch) {
    WDGS_REQUIRE(r, WDGS_E_INVALID, "wdgs_mesh_rasterizer_stats: null argument");
    WDGS_REQUIRE(r->encoded, WDGS_E_STATE, "rasterizeMesh: no encode precedes the read of its statistics");
    wdgs_device* d = r->dev;
    WDGS_REQUIRE(!d->capturing, WDGS_E_STATE, "rasterizeMesh: the read of the statistics waits and cannot be recorded into a command buffer");
    u32 host[MR_S_WORDS];
    WDGS_CHECK_HIP(hipMemcpyAsync(host, r->stats, sizeof(host), hipMemcpyDeviceToHost, d->stream));
    WDGS_CHECK_HIP(wdgs_sync_lanes(d));
    uint32_t* const outs[8] = {invalid_faces, clipped_faces, degenerate_faces, culled_faces, empty_faces, rasterized_faces, covered_pixels, viewport_mismatch};
    for (u32 k = 0; k < 8u; k++) {
        if (outs[k]) *outs[k] = host[k];
    }
    return WDGS_OK;
}

extern "C" int wdgs_depth_agreement(wdgs_device* dev, const void* a_f32_dev, const void* b_f32_dev, const void* b_weight_sum_f32_dev, float min_weight_sum, uint32_t width,
                                    uint32_t height, float max_difference, float threshold, void* out_u64x5_dev) {
    WDGS_REQUIRE(dev && a_f32_dev && b_f32_dev && out_u64x5_dev, WDGS_E_INVALID, "wdgs_depth_agreement: null argument");
    WDGS_REQUIRE(width >= 1u && width <= WDGS_MESH_RASTER_MAX_SIZE && height >= 1u && height <= WDGS_MESH_RASTER_MAX_SIZE, WDGS_E_INVALID,
                 "wdgs_depth_agreement: bad image size %ux%u", width, height);
    WDGS_REQUIRE(positive_finite(max_difference) && positive_finite(threshold) && threshold <= max_difference, WDGS_E_INVALID,
                 "depthAgreement: 0 < threshold <= max_difference, both finite (got %g, %g)", (double)threshold, (double)max_difference);
    WDGS_REQUIRE((((uintptr_t)a_f32_dev | (uintptr_t)b_f32_dev | (uintptr_t)b_weight_sum_f32_dev) & 3u) == 0u && ((uintptr_t)out_u64x5_dev & 7u) == 0u, WDGS_E_INVALID,
                 "wdgs_depth_agreement: misaligned argument");
    WDGS_CHECK_HIP(hipMemsetAsync(out_u64x5_dev, 0, 40, dev->stream));
    const u32 n = width * height;
    const u32 grid = std::min<u32>(ceil_div(n, MR_THREADS), (u32)dev->num_cus * 4u);
    WDGS_LAUNCH(dev, "depth_agreement", depth_agreement_kernel, dim3(grid), dim3(MR_THREADS), 0, static_cast<const float*>(a_f32_dev), static_cast<const float*>(b_f32_dev),
                static_cast<const float*>(b_weight_sum_f32_dev), min_weight_sum, n, max_difference, threshold, static_cast<u64*>(out_u64x5_dev));
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}
