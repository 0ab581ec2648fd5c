// A texture atlas of a mesh baked from photographs (no counterpart in the reference, which renders splats only).  include/webdgs.h
// states the definition operation by operation; tests/meshtexture_ref.py restates it.
//
// The atlas is arithmetic in (F, C): square cells of C x C texels, two faces per cell, the even face below the anti-diagonal and the odd one above it, turned
// by 180 degrees.  The state is one 16-byte row {R, G, B, Wsum} of u32 per texel, CELL-major (row = cell C C + j C + i), so that the rows a wave touches are
// contiguous.  One accumulate call is one view and one thread owns a texel at a time.  A wave takes 8 or 10 consecutive cells.  What all texels of a face
// share -- three indices, three gathered vertices, the view transform, the projection of the corners, the normal, the cosine at the corners -- is done once,
// by three lanes per face, for all 16 or 20 faces of the wave at once; ballots turn it into wave-uniform face masks, and the wave then walks its texels 64 at
// a time, handing the corners and the normal to the texel lanes with shuffles.  A chunk none of whose faces passes the face-level tests costs one scalar test,
// and a wave with no such face leaves before it touches a row or an image texel: a typical view sees a small part of a mesh, and what such a face costs is
// its 12 bytes of indices and 36 of positions.  A texel that drops out on the way never
// touches its row.  Integer sums: the state does not depend on the order of the views and every byte is a function of the inputs.
//
// Section 16's to 22's rule holds: no spin-wait, no inter-workgroup flag, no look-back, no grid barrier, no float atomics; what one launch writes the next one
// reads.  The only atomics are the integer adds of the per-workgroup totals, to words no kernel reads.
#include <algorithm>
#include <memory>
#include <vector>

#include "dmath.h"
#include "launch.h"

namespace {

typedef unsigned long long u64;

constexpr u32 MT_THREADS = 256;
constexpr u32 MT_WAVES = MT_THREADS / 64;
// The totals, u64 words, kept as section 22 keeps them: MT_SLOTS partial sums of one 128-byte line each, workgroup b adds to slot b mod MT_SLOTS, stats sums
// the slots.  Words of a slot: the seven the accumulate kernel counts, in the order of the definition, then (slot 0 only) the calls whose camera block was of
// another image size.  A second set of slots, cleared by every resolve, holds the baked, filled and fallback texels in words 0 to 2.
constexpr u32 MT_SLOTS = 64, MT_SLOT_WORDS = 16;
constexpr u32 MT_COUNTS = 7, MT_T_MISMATCH = 7, MT_RESOLVE_COUNTS = 3;
constexpr u32 MT_T_RESOLVE_SLOTS = MT_SLOTS * MT_SLOT_WORDS, MT_T_WORDS = 2 * MT_SLOTS * MT_SLOT_WORDS;
constexpr u32 MT_MAX_ACCUMULATES = 65535;

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) < __builtin_inff(); }

__device__ __forceinline__ bool depth_agrees(float z, float d, float tolerance) { return d > 0.0f && d < __builtin_inff() && fabsf(z - d) <= tolerance; }

// Per workgroup: the waves' counts (wave-uniform) summed by thread k, one atomic per total
template <u32 N>
__device__ __forceinline__ void add_totals(const u32 (&counts)[N], u64* __restrict__ slots) {
    __shared__ u32 s_counts[N][MT_WAVES];
    if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
        for (u32 k = 0; k < N; k++) s_counts[k][threadIdx.x >> 6] = counts[k];
    }
    __syncthreads();
    if (threadIdx.x < N) {
        const u32 s = (s_counts[threadIdx.x][0] + s_counts[threadIdx.x][1]) + (s_counts[threadIdx.x][2] + s_counts[threadIdx.x][3]);
        if (s != 0u)
            (void)__hip_atomic_fetch_add(slots + (blockIdx.x % MT_SLOTS) * MT_SLOT_WORDS + threadIdx.x, (u64)s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Step 4's Q for the view-space point p of a face with normal n, nn = n . n
__device__ __forceinline__ u32 weight_q(float nx, float ny, float nz, float nn, float px, float py, float pz, float min_cos, bool two_sided) {
    const float dot = (nx * px + ny * py) + nz * pz;
    const float pp = (px * px + py * py) + pz * pz;
    float c = wd_div(-dot, wd_sqrt(nn * pp));
    if (two_sided) c = fabsf(c);
    return (finite_f(c) && !(c < min_cos)) ? (u32)(i32)__builtin_rintf((c > 1.0f ? 1.0f : c) * 256.0f) : 0u;
}

// The texel of thread T in the cell-major order: its cell, its place (i, j) in the cell, which face of the cell owns it and its place (i', j') in that
// face's chart
template <u32 C>
struct Texel {
    u32 cell, i, j, ip, jp;
    bool odd, owned;
    __device__ __forceinline__ explicit Texel(u32 T) {
        cell = T / (C * C);
        const u32 local = T % (C * C);
        i = local % C;
        j = local / C;
        const u32 s = i + j;
        odd = s >= C;
        owned = s != C - 1u;
        ip = odd ? C - 1u - i : i;
        jp = odd ? C - 1u - j : j;
    }
    __device__ __forceinline__ u32 face() const { return 2u * cell + (odd ? 1u : 0u); }   // (cell < 2^22: no overflow)
};

// The cells one wave takes: 8 of 16 texels (16 faces, 48 corner lanes, 2 chunks of 64 texels) or 10 of 64, 256, 1024 texels (20 faces, 60 corner lanes, 10, 40,
// 160 chunks).  One wave per cell -- the first build -- spent 300 us on a view that sees none of 2 M faces: the face-level work of a wave, some two hundred
// vector instructions, was paid per cell.  Here it is paid once per 8 or 10 cells, and a dead cell costs a scalar test.
template <u32 C>
struct Batch {
    static constexpr u32 CC = C * C;
    static constexpr u32 CELLS = C == 4u ? 8u : 10u;
    static constexpr u32 FACES = 2u * CELLS;
    static constexpr u32 CHUNKS = CELLS * CC / 64u;
    static constexpr u32 CELLS_PER_CHUNK = CC >= 64u ? 1u : 64u / CC;
    // bit 3 f of a face mask belongs to face f of the wave: the faces of one chunk's cells
    static constexpr u64 CHUNK_FACES = 0x249249249249249ull & ((1ull << (6u * CELLS_PER_CHUNK)) - 1ull);
};

// all three corners of a face: bit 3 f of the result is bit 3 f & bit 3 f + 1 & bit 3 f + 2 of the ballot
__device__ __forceinline__ u64 all_three(u64 b) { return b & (b >> 1) & (b >> 2); }

template <u32 C, bool DEPTH>
__global__ __launch_bounds__(MT_THREADS) void texture_accumulate_kernel(const float* __restrict__ vertices, u32 V, const u32* __restrict__ faces, u32 F,
                                                                        const float* __restrict__ camera, const u32* __restrict__ image,
                                                                        const float* __restrict__ mesh_depth, u32 W, u32 H, float near, float depth_tolerance,
                                                                        float min_cos, u32 two_sided, u32* __restrict__ rows, u64* __restrict__ totals) {
    if (!(camera[64] == (float)W && camera[65] == (float)H)) {   // (uniform: a camera block of another image size accumulates nothing)
        if (blockIdx.x == 0u && threadIdx.x == 0u) (void)__hip_atomic_fetch_add(totals + MT_T_MISMATCH, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    typedef Batch<C> B;
    constexpr u32 CC = B::CC, M = C - 3u;
    const u32 lane = threadIdx.x & 63u;
    const u32 first_cell = (blockIdx.x * MT_WAVES + (threadIdx.x >> 6)) * B::CELLS;   // (at most 2^24 cells: no overflow)
    const u32 first_face = 2u * first_cell;
    const u32 wave_faces = first_face < F ? min(F - first_face, B::FACES) : 0u;

    // A. Lane 3 f + k takes corner k of the wave's f-th face: mr_vertices_kernel's arithmetic (meshraster.hip) and the projection
    float vx = 0.0f, vy = 0.0f, z = 0.0f;
    bool valid = false, left = false, right = false, above = false, below = false;
    if (lane < 3u * wave_faces) {
        const u32 index = faces[3u * (size_t)first_face + lane];
        if (index < V) {
            const float px = vertices[3u * (size_t)index], py = vertices[3u * (size_t)index + 1u], pz = vertices[3u * (size_t)index + 2u];
            vx = ((camera[0] * px + camera[4] * py) + camera[8] * pz) + camera[12];
            vy = ((camera[1] * px + camera[5] * py) + camera[9] * pz) + camera[13];
            z = ((camera[2] * px + camera[6] * py) + camera[10] * pz) + camera[14];
            valid = finite_f(vx) && finite_f(vy) && finite_f(z) && z >= near;
            if (valid) {
                const float sx = (wd_div(camera[32] * vx, z) * 0.5f + 0.5f) * (float)W;
                const float sy = (wd_div((-camera[37]) * vy, z) * 0.5f + 0.5f) * (float)H;
                left = sx < 0.0f;
                right = sx > (float)W;
                above = sy < 0.0f;
                below = sy > (float)H;
            }
        }
    }
    // the faces by class -- invalid, else facing away at every corner, else off one side of the image at every corner, else live -- as masks with bit 3 f
    // for face f; the texels: usable, in the image, visible, accumulated.  All wave-uniform
    const u64 exist = wave_faces ? 0x249249249249249ull & ((1ull << (3u * wave_faces)) - 1ull) : 0ull;
    const u64 good = all_three(__ballot(valid)) & exist;
    u32 counts[MT_COUNTS] = {(u32)__popcll(exist & ~good), 0u, 0u, 0u, 0u, 0u, 0u};
    if (good != 0ull) {   // (a wave all of whose faces are invalid -- behind the camera -- leaves here)
        // B. The corner lanes of a face exchange their corners: the face's normal, and the weight the view would have at the lane's own corner
        const u32 base = (lane / 3u) * 3u;
        float q[3][3];
#pragma unroll
        for (u32 k = 0; k < 3u; k++) {
            q[k][0] = __shfl(vx, (int)((base + k) & 63u));
            q[k][1] = __shfl(vy, (int)((base + k) & 63u));
            q[k][2] = __shfl(z, (int)((base + k) & 63u));
        }
        const float ax = q[1][0] - q[0][0], ay = q[1][1] - q[0][1], az = q[1][2] - q[0][2];
        const float bx = q[2][0] - q[0][0], by = q[2][1] - q[0][1], bz = q[2][2] - q[0][2];
        const float nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
        const float nn = (nx * nx + ny * ny) + nz * nz;
        const bool away = weight_q(nx, ny, nz, nn, vx, vy, z, min_cos, two_sided != 0u) == 0u;
        const u64 facing_away = all_three(__ballot(away)) & good;
        const u64 off_image = (all_three(__ballot(left)) | all_three(__ballot(right)) | all_three(__ballot(above)) | all_three(__ballot(below))) & good & ~facing_away;
        const u64 live = good & ~facing_away & ~off_image;
        counts[1] = (u32)__popcll(facing_away);
        counts[2] = (u32)__popcll(off_image);

        // C. The wave's texels, 64 at a time; a chunk none of whose faces is live touches no row and no image texel
        if (live != 0ull) {
#pragma unroll 1
            for (u32 chunk = 0; chunk < B::CHUNKS; chunk++) {
                const u32 chunk_cell = chunk * 64u / CC;   // the first (for C >= 8: the only) cell of the chunk, counted from the wave's first
                if (((live >> (6u * chunk_cell)) & B::CHUNK_FACES) == 0ull) continue;   // (uniform)
                const u32 t_wave = chunk * 64u + lane;
                const Texel<C> t(t_wave);   // (its cell counts from the wave's first)
                const u32 shift = 3u * t.face();   // (at most 57)
                float P[3][3];
#pragma unroll
                for (u32 k = 0; k < 3u; k++) {
                    P[k][0] = __shfl(vx, (int)(shift + k));
                    P[k][1] = __shfl(vy, (int)(shift + k));
                    P[k][2] = __shfl(z, (int)(shift + k));
                }
                const float fnx = __shfl(nx, (int)shift), fny = __shfl(ny, (int)shift), fnz = __shfl(nz, (int)shift), fnn = __shfl(nn, (int)shift);
                bool flags[4] = {false, false, false, false};   // usable, in the image, visible, accumulated
                if (t.owned && ((live >> shift) & 1ull) != 0ull) {
                    // 2. the texel's point on the face's plane, and its projection
                    const float u = wd_div((float)t.ip, (float)M), v = wd_div((float)t.jp, (float)M);
                    const float w = (1.0f - u) - v;
                    const float px = (w * P[0][0] + u * P[1][0]) + v * P[2][0];
                    const float py = (w * P[0][1] + u * P[1][1]) + v * P[2][1];
                    const float pz = (w * P[0][2] + u * P[1][2]) + v * P[2][2];
                    const float sx = (wd_div(camera[32] * px, pz) * 0.5f + 0.5f) * (float)W;
                    const float sy = (wd_div((-camera[37]) * py, pz) * 0.5f + 0.5f) * (float)H;
                    flags[0] = finite_f(px) && finite_f(py) && finite_f(pz) && pz >= near && finite_f(sx) && finite_f(sy) && fabsf(sx) <= 16384.0f && fabsf(sy) <= 16384.0f;
                    if (flags[0]) {
                        const u32 xs = (u32)((i32)__builtin_rintf(sx * 256.0f) - 128), ys = (u32)((i32)__builtin_rintf(sy * 256.0f) - 128);
                        flags[1] = xs <= 256u * (W - 1u) && ys <= 256u * (H - 1u);
                        if (flags[1]) {
                            const u32 i0 = xs >> 8, a = xs & 255u, i1 = min(i0 + 1u, W - 1u);
                            const u32 j0 = ys >> 8, b = ys & 255u, j1 = min(j0 + 1u, H - 1u);
                            const u32 at[4] = {j0 * W + i0, j0 * W + i1, j1 * W + i0, j1 * W + i1};   // (W H <= 2^26)
                            // 3. occlusion: all four texels of the mesh's own depth image hold this depth
                            flags[2] = true;
                            if (DEPTH) {
                                float d[4];
#pragma unroll
                                for (u32 k = 0; k < 4u; k++) d[k] = mesh_depth[at[k]];
#pragma unroll
                                for (u32 k = 0; k < 4u; k++) flags[2] = flags[2] && depth_agrees(pz, d[k], depth_tolerance);
                            }
                            if (flags[2]) {
                                // 4. the weight
                                const u32 Q = weight_q(fnx, fny, fnz, fnn, px, py, pz, min_cos, two_sided != 0u);
                                flags[3] = Q != 0u;
                                if (flags[3]) {
                                    // 5. the sample, integers only, rounded to a byte: S <= 65536 x 255
                                    u32 texel[4];
#pragma unroll
                                    for (u32 k = 0; k < 4u; k++) texel[k] = image[at[k]];
                                    const u32 wt[4] = {(256u - a) * (256u - b), a * (256u - b), (256u - a) * b, a * b};
                                    u32 add[3];
#pragma unroll
                                    for (u32 ch = 0; ch < 3u; ch++) {
                                        u32 S = 0u;
#pragma unroll
                                        for (u32 k = 0; k < 4u; k++) S += wt[k] * ((texel[k] >> (8u * ch)) & 255u);
                                        add[ch] = Q * ((S + 32768u) >> 16);
                                    }
                                    // 6. the row is this thread's alone: one 16-byte load, one 16-byte store
                                    uint4* row = reinterpret_cast<uint4*>(rows) + ((size_t)first_cell * CC + t_wave);
                                    uint4 r = *row;
                                    r.x += add[0];
                                    r.y += add[1];
                                    r.z += add[2];
                                    r.w += Q;
                                    *row = r;
                                }
                            }
                        }
                    }
                }
#pragma unroll
                for (u32 k = 0; k < 4u; k++) counts[3u + k] += (u32)__popcll(__ballot(flags[k]));
            }
        }
    }
    add_totals(counts, totals);
}

__device__ __forceinline__ u32 baked_colour(uint4 r) {
    const u32 half = r.w >> 1;
    return min((r.x + half) / r.w, 255u) | (min((r.y + half) / r.w, 255u) << 8) | (min((r.z + half) / r.w, 255u) << 16) | 0xFF000000u;
}

// One thread per texel of the whole atlas, cell-major: every texel of texture_out and state_out is written
template <u32 C>
__global__ __launch_bounds__(MT_THREADS) void texture_resolve_kernel(const u32* __restrict__ rows, const u32* __restrict__ faces, u32 F, u32 V,
                                                                     const u32* __restrict__ colours, u32 cells_per_row, u32 atlas_texels, u32 min_weight, u32 fill,
                                                                     u32* __restrict__ texture_out, unsigned char* __restrict__ state_out, u64* __restrict__ totals) {
    constexpr u32 M = C - 3u;
    const u32 T = blockIdx.x * MT_THREADS + threadIdx.x;
    bool flags[MT_RESOLVE_COUNTS] = {false, false, false};   // baked, filled, fallback
    if (T < atlas_texels) {
        const Texel<C> t(T);
        const u32 face = t.face();
        u32 colour = 0u, state = 0u;
        if (t.owned && face < F) {
            const uint4* row = reinterpret_cast<const uint4*>(rows) + T;
            const u32 threshold = max(min_weight, 1u);
            const uint4 r = *row;
            if (r.w >= threshold) {
                colour = baked_colour(r);
                state = 1u;
                flags[0] = true;
            } else {
                u32 n = 0u, sum[3] = {0u, 0u, 0u};
                if (fill != 0u) {
#pragma unroll
                    for (i32 dj = -1; dj <= 1; dj++) {
#pragma unroll
                        for (i32 di = -1; di <= 1; di++) {
                            if (di == 0 && dj == 0) continue;
                            const u32 ni = t.i + (u32)di, nj = t.j + (u32)dj;   // (wraps below 0: fails the next test)
                            if (ni >= C || nj >= C) continue;
                            const u32 s = ni + nj;
                            if (t.odd ? s < C : s > C - 2u) continue;   // (another face's texel, or nobody's)
                            const uint4 o = row[dj * (i32)C + di];
                            if (o.w >= threshold) {
                                const u32 c = baked_colour(o);
                                sum[0] += c & 255u;
                                sum[1] += (c >> 8) & 255u;
                                sum[2] += (c >> 16) & 255u;
                                n++;
                            }
                        }
                    }
                }
                if (n != 0u) {
                    colour = ((sum[0] + n / 2u) / n) | (((sum[1] + n / 2u) / n) << 8) | (((sum[2] + n / 2u) / n) << 16) | 0xFF000000u;
                    state = 2u;
                    flags[1] = true;
                } else {
                    // the vertex colours mixed with the clamped integer barycentrics; a corner without a colour counts as zeros
                    const u32 i2 = min(t.ip, M), j2 = min(t.jp, M - i2), k2 = M - i2 - j2;
                    u32 c[3] = {0u, 0u, 0u};
                    if (colours) {
#pragma unroll
                        for (u32 k = 0; k < 3u; k++) {
                            const u32 index = faces[3u * (size_t)face + k];
                            if (index < V) c[k] = colours[index];
                        }
                    }
                    colour = 0xFF000000u;
#pragma unroll
                    for (u32 ch = 0; ch < 3u; ch++)
                        colour |= (((k2 * ((c[0] >> (8u * ch)) & 255u) + i2 * ((c[1] >> (8u * ch)) & 255u)) + j2 * ((c[2] >> (8u * ch)) & 255u) + M / 2u) / M) << (8u * ch);
                    flags[2] = true;
                }
            }
        }
        const u32 x = (t.cell % cells_per_row) * C + t.i, y = (t.cell / cells_per_row) * C + t.j;
        const size_t at = (size_t)y * (cells_per_row * C) + x;
        texture_out[at] = colour;
        if (state_out) state_out[at] = (unsigned char)state;
    }
    const u32 counts[MT_RESOLVE_COUNTS] = {(u32)__popcll(__ballot(flags[0])), (u32)__popcll(__ballot(flags[1])), (u32)__popcll(__ballot(flags[2]))};
    add_totals(counts, totals + MT_T_RESOLVE_SLOTS);
}

bool aligned4(const void* p) { return ((uintptr_t)p & 3u) == 0u; }

}  // namespace

// ---------------------------------------------------------------- launchers
int launch_mesh_texture_accumulate(wdgs_device* dev, u32 cell, const float* vertices, u32 V, const u32* faces, u32 F, const float* camera, const u32* image,
                                   const float* mesh_depth, u32 W, u32 H, float near, float depth_tolerance, float min_cos, u32 two_sided, u32* rows,
                                   unsigned long long* totals) {
    const u32 cells = (F + 1u) / 2u, cells_per_workgroup = MT_WAVES * (cell == 4u ? Batch<4>::CELLS : Batch<8>::CELLS);
    const dim3 grid(std::max(ceil_div(cells, cells_per_workgroup), 1u)), block(MT_THREADS);   // (one workgroup also for no faces: the camera block is still looked at)
#define MT_LAUNCH(C, D)                                                                                                                                   \
    WDGS_LAUNCH(dev, "mesh_texture_accumulate", (texture_accumulate_kernel<C, D>), grid, block, 0, vertices, V, faces, F, camera, image, mesh_depth, W, H, near, \
                depth_tolerance, min_cos, two_sided, rows, totals)
#define MT_LAUNCH_C(C)                 \
    do {                               \
        if (mesh_depth) MT_LAUNCH(C, true); \
        else MT_LAUNCH(C, false);      \
    } while (0)
    if (cell == 4u) MT_LAUNCH_C(4u);
    else if (cell == 8u) MT_LAUNCH_C(8u);
    else if (cell == 16u) MT_LAUNCH_C(16u);
    else MT_LAUNCH_C(32u);
#undef MT_LAUNCH_C
#undef MT_LAUNCH
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

int launch_mesh_texture_resolve(wdgs_device* dev, u32 cell, const u32* rows, const u32* faces, u32 F, u32 V, const u32* colours, u32 cells_per_row, u32 atlas_rows,
                                u32 min_weight, u32 fill, u32* texture_out, unsigned char* state_out, unsigned long long* totals) {
    WDGS_CHECK_HIP(hipMemsetAsync(totals + MT_T_RESOLVE_SLOTS, 0, sizeof(u64) * MT_SLOTS * MT_SLOT_WORDS, dev->stream));
    const u32 atlas_texels = cells_per_row * atlas_rows * cell * cell;
    if (atlas_texels != 0u) {
        const dim3 grid(ceil_div(atlas_texels, MT_THREADS)), block(MT_THREADS);
#define MT_LAUNCH(C)                                                                                                                                           \
    WDGS_LAUNCH(dev, "mesh_texture_resolve", (texture_resolve_kernel<C>), grid, block, 0, rows, faces, F, V, colours, cells_per_row, atlas_texels, min_weight, fill, \
                texture_out, state_out, totals)
        if (cell == 4u) MT_LAUNCH(4u);
        else if (cell == 8u) MT_LAUNCH(8u);
        else if (cell == 16u) MT_LAUNCH(16u);
        else MT_LAUNCH(32u);
#undef MT_LAUNCH
    }
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

// ---------------------------------------------------------------- the C ABI object (include/webdgs.h)
struct wdgs_mesh_texture_baker {
    wdgs_device* dev = nullptr;
    DevMem<u32> rows;      // [cells C C][4]
    DevMem<u64> totals;    // MT_T_WORDS
    size_t capacity_texels = 0;
    u32 F = 0, cell = 0, cells = 0, cells_per_row = 0, atlas_rows = 0;
    u32 accumulates = 0;   // since the reset, in host arithmetic on the calls made
    bool sized = false;
};

extern "C" int wdgs_mesh_texture_baker_create(wdgs_device* dev, wdgs_mesh_texture_baker** out) {
    WDGS_REQUIRE(dev && out, WDGS_E_INVALID, "wdgs_mesh_texture_baker_create: null argument");
    WDGS_REQUIRE(!dev->capturing, WDGS_E_STATE, "wdgs_mesh_texture_baker_create while recording a command buffer");
    auto b = std::make_unique<wdgs_mesh_texture_baker>();
    b->dev = dev;
    WDGS_TRY(b->totals.alloc(MT_T_WORDS, true, dev->stream));
    *out = b.release();
    return WDGS_OK;
}

extern "C" int wdgs_mesh_texture_baker_destroy(wdgs_mesh_texture_baker* b) {
    if (!b) return WDGS_OK;
    if (wdgs_device_alive(b->dev) && !b->dev->capturing) (void)wdgs_sync_lanes(b->dev);
    delete b;
    return WDGS_OK;
}

extern "C" int wdgs_mesh_texture_baker_reset(wdgs_mesh_texture_baker* b, uint32_t num_faces, uint32_t cell, uint32_t accumulates) {
    WDGS_REQUIRE(b, WDGS_E_INVALID, "wdgs_mesh_texture_baker_reset: null argument");
    WDGS_REQUIRE(num_faces < (1u << 31), WDGS_E_INVALID, "bakeTexture: %u faces, 2^31 or more", num_faces);
    WDGS_REQUIRE(cell == 4u || cell == 8u || cell == 16u || cell == 32u, WDGS_E_INVALID, "bakeTexture: a cell of %u texels (4, 8, 16 or 32)", cell);
    // the layout, in integers: cells_per_row = ceil(sqrt(cells))
    const u32 cells = (num_faces + 1u) / 2u;
    u32 per_row = 0;
    while ((u64)per_row * per_row < cells) per_row++;
    const u32 atlas_rows = per_row ? ceil_div(cells, per_row) : 0u;
    WDGS_REQUIRE((u64)per_row * cell <= WDGS_MESH_TEXTURE_MAX_SIZE, WDGS_E_INVALID, "bakeTexture: %u faces in cells of %u texels need an atlas %llu texels wide (at most %u)",
                 num_faces, cell, (unsigned long long)per_row * cell, WDGS_MESH_TEXTURE_MAX_SIZE);
    WDGS_REQUIRE(accumulates <= MT_MAX_ACCUMULATES, WDGS_E_INVALID, "bakeTexture: a count of %u accumulates (at most %u)", accumulates, MT_MAX_ACCUMULATES);
    wdgs_device* d = b->dev;
    WDGS_REQUIRE(!d->capturing, WDGS_E_STATE, "bakeTexture: a reset cannot be recorded into a command buffer");
    const size_t texels = (size_t)cells * cell * cell;   // (at most 2^28)
    if (texels > b->capacity_texels) {
        WDGS_CHECK_HIP(wdgs_sync_lanes(d));   // (nothing in flight may still read the block given back)
        b->capacity_texels = 0;
        b->sized = false;
        WDGS_TRY(b->rows.alloc(4 * texels, false, d->stream));
        b->capacity_texels = texels;
    }
    if (texels != 0) WDGS_CHECK_HIP(hipMemsetAsync(b->rows, 0, 16 * texels, d->stream));
    WDGS_CHECK_HIP(hipMemsetAsync(b->totals, 0, sizeof(u64) * MT_T_WORDS, d->stream));
    b->F = num_faces;
    b->cell = cell;
    b->cells = cells;
    b->cells_per_row = per_row;
    b->atlas_rows = atlas_rows;
    b->accumulates = accumulates;
    b->sized = true;
    return WDGS_OK;
}

extern "C" int wdgs_mesh_texture_baker_layout(wdgs_mesh_texture_baker* b, uint32_t* width, uint32_t* height, uint32_t* cells_per_row) {
    WDGS_REQUIRE(b, WDGS_E_INVALID, "wdgs_mesh_texture_baker_layout: null argument");
    WDGS_REQUIRE(b->sized, WDGS_E_STATE, "bakeTexture: no reset precedes the layout");
    if (width) *width = b->cells_per_row * b->cell;
    if (height) *height = b->atlas_rows * b->cell;
    if (cells_per_row) *cells_per_row = b->cells_per_row;
    return WDGS_OK;
}

extern "C" int wdgs_mesh_texture_baker_accumulate(wdgs_mesh_texture_baker* b, const void* vertices_f32_dev, uint32_t num_vertices, const void* faces_u32_dev,
                                                  uint32_t num_faces, const void* camera_dev, const void* image_rgba8_dev, const void* mesh_depth_f32_dev, uint32_t width,
                                                  uint32_t height, float near, float depth_tolerance, float min_cos, uint32_t two_sided) {
    WDGS_REQUIRE(b, WDGS_E_INVALID, "wdgs_mesh_texture_baker_accumulate: null argument");
    WDGS_REQUIRE(b->sized, WDGS_E_STATE, "bakeTexture: no reset precedes the accumulate");
    WDGS_REQUIRE(num_faces == b->F, WDGS_E_STATE, "bakeTexture: %u faces, the reset was for %u", num_faces, b->F);
    WDGS_REQUIRE(b->accumulates < MT_MAX_ACCUMULATES, WDGS_E_STATE, "bakeTexture: %u views accumulated since the reset, one more could overflow a sum", b->accumulates);
    WDGS_REQUIRE(num_vertices < (1u << 31), WDGS_E_INVALID, "bakeTexture: %u vertices, 2^31 or more", num_vertices);
    WDGS_REQUIRE(width >= 1u && width <= WDGS_MESH_RASTER_MAX_SIZE && height >= 1u && height <= WDGS_MESH_RASTER_MAX_SIZE, WDGS_E_INVALID,
                 "bakeTexture: bad image size %ux%u (1 to %u)", width, height, WDGS_MESH_RASTER_MAX_SIZE);
    WDGS_REQUIRE(near > 0.0f && near < __builtin_inff(), WDGS_E_INVALID, "bakeTexture: near %g must be positive and finite", (double)near);
    WDGS_REQUIRE(depth_tolerance >= 0.0f && depth_tolerance < __builtin_inff(), WDGS_E_INVALID, "bakeTexture: depth tolerance %g must be finite and not negative",
                 (double)depth_tolerance);
    WDGS_REQUIRE(min_cos >= 0.0f && min_cos <= 1.0f, WDGS_E_INVALID, "bakeTexture: min_cos %g is not in [0, 1]", (double)min_cos);
    WDGS_REQUIRE(camera_dev && image_rgba8_dev && (num_faces == 0 || faces_u32_dev) && (num_faces == 0 || num_vertices == 0 || vertices_f32_dev), WDGS_E_INVALID,
                 "wdgs_mesh_texture_baker_accumulate: null vertices, faces, camera or image");
    WDGS_REQUIRE(aligned4(vertices_f32_dev) && aligned4(faces_u32_dev) && aligned4(camera_dev) && aligned4(image_rgba8_dev) && aligned4(mesh_depth_f32_dev), WDGS_E_INVALID,
                 "wdgs_mesh_texture_baker_accumulate: misaligned buffer");
    WDGS_TRY(launch_mesh_texture_accumulate(b->dev, b->cell, static_cast<const float*>(vertices_f32_dev), num_vertices, static_cast<const u32*>(faces_u32_dev), num_faces,
                                            static_cast<const float*>(camera_dev), static_cast<const u32*>(image_rgba8_dev), static_cast<const float*>(mesh_depth_f32_dev),
                                            width, height, near, depth_tolerance, min_cos, two_sided, b->rows, b->totals));
    b->accumulates++;
    return WDGS_OK;
}

extern "C" int wdgs_mesh_texture_baker_resolve(wdgs_mesh_texture_baker* b, const void* faces_u32_dev, uint32_t num_faces, uint32_t num_vertices,
                                               const void* colours_rgba8_dev, void* texture_out_rgba8_dev, void* state_out_u8_dev, uint32_t min_weight, uint32_t fill) {
    WDGS_REQUIRE(b, WDGS_E_INVALID, "wdgs_mesh_texture_baker_resolve: null argument");
    WDGS_REQUIRE(b->sized, WDGS_E_STATE, "bakeTexture: no reset precedes the resolve");
    WDGS_REQUIRE(num_faces == b->F, WDGS_E_STATE, "bakeTexture: %u faces, the reset was for %u", num_faces, b->F);
    WDGS_REQUIRE(num_vertices < (1u << 31), WDGS_E_INVALID, "bakeTexture: %u vertices, 2^31 or more", num_vertices);
    WDGS_REQUIRE(num_faces == 0 || (faces_u32_dev && texture_out_rgba8_dev), WDGS_E_INVALID, "wdgs_mesh_texture_baker_resolve: null faces or texture output");
    WDGS_REQUIRE(aligned4(faces_u32_dev) && aligned4(colours_rgba8_dev) && aligned4(texture_out_rgba8_dev), WDGS_E_INVALID,
                 "wdgs_mesh_texture_baker_resolve: misaligned buffer");
    return launch_mesh_texture_resolve(b->dev, b->cell, b->rows, static_cast<const u32*>(faces_u32_dev), num_faces, num_vertices, static_cast<const u32*>(colours_rgba8_dev),
                                       b->cells_per_row, b->atlas_rows, min_weight, fill, static_cast<u32*>(texture_out_rgba8_dev),
                                       static_cast<unsigned char*>(state_out_u8_dev), b->totals);
}

extern "C" int wdgs_mesh_texture_baker_read(wdgs_mesh_texture_baker* b, uint32_t* rows_out) {
    WDGS_REQUIRE(b, WDGS_E_INVALID, "wdgs_mesh_texture_baker_read: null argument");
    WDGS_REQUIRE(b->sized, WDGS_E_STATE, "bakeTexture: no reset precedes the read");
    wdgs_device* d = b->dev;
    WDGS_REQUIRE(!d->capturing, WDGS_E_STATE, "bakeTexture: the read of the state waits and cannot be recorded into a command buffer");
    const size_t texels = (size_t)b->cells * b->cell * b->cell;
    if (texels != 0 && rows_out) WDGS_CHECK_HIP(hipMemcpyAsync(rows_out, b->rows, 16 * texels, hipMemcpyDeviceToHost, d->stream));
    WDGS_CHECK_HIP(wdgs_sync_lanes(d));
    return WDGS_OK;
}

extern "C" int wdgs_mesh_texture_baker_stats(wdgs_mesh_texture_baker* b, uint64_t* out11) {
    WDGS_REQUIRE(b && out11, WDGS_E_INVALID, "wdgs_mesh_texture_baker_stats: null argument");
    WDGS_REQUIRE(b->sized, WDGS_E_STATE, "bakeTexture: no reset precedes the read of its statistics");
    wdgs_device* d = b->dev;
    WDGS_REQUIRE(!d->capturing, WDGS_E_STATE, "bakeTexture: the read of the statistics waits and cannot be recorded into a command buffer");
    std::vector<u64> host(MT_T_WORDS);
    WDGS_CHECK_HIP(hipMemcpyAsync(host.data(), b->totals, sizeof(u64) * MT_T_WORDS, hipMemcpyDeviceToHost, d->stream));
    WDGS_CHECK_HIP(wdgs_sync_lanes(d));
    for (u32 k = 0; k < MT_COUNTS + 1u + MT_RESOLVE_COUNTS; k++) {   // (the slots of a total summed; the last three from the resolve's set)
        const u32 word = k <= MT_T_MISMATCH ? k : MT_T_RESOLVE_SLOTS + (k - MT_T_MISMATCH - 1u);
        u64 sum = 0;
        for (u32 s = 0; s < MT_SLOTS; s++) sum += host[word + s * MT_SLOT_WORDS];
        out11[k] = sum;
    }
    return WDGS_OK;
}
