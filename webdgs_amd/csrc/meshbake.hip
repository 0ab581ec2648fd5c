// Vertex colours of a mesh baked from photographs (no counterpart in the reference, which renders splats only).  include/webdgs.h
// states the definition operation by operation; tests/meshbake_ref.py restates it.
//
// One accumulate call is one view.  One thread owns one vertex: it projects it with the mesh rasterizer's VERTEX rule, tests the four texels round it against
// the mesh's own depth image of that view, weighs the view by the cosine between the vertex normal and the direction to the camera, samples the photograph
// bilinearly in integers and adds {Q s_r, Q s_g, Q s_b, Q} to the vertex's row of u64 sums.  The row belongs to that thread alone, so the add is two 16-byte
// loads and two 16-byte stores, and a vertex that drops out on the way never touches its row: most of a mesh is not seen by a typical view, and what those
// vertices cost is their 12 bytes of position.  A sum of integers does not depend on the order of the views, so every byte is a function of the inputs.
//
// Section 16's to 21's rule holds: no spin-wait, no inter-workgroup flag, no look-back, no grid barrier, no float atomics; what one launch writes the next one
// reads.  The only atomics are the integer adds of the per-workgroup totals, to words no kernel reads.
#include <algorithm>
#include <memory>
#include <vector>

#include "dmath.h"
#include "launch.h"

namespace {

typedef unsigned long long u64;

constexpr u32 MB_THREADS = 256;
constexpr u32 MB_WAVES = MB_THREADS / 64;
// The totals, u64 words.  A total is kept as MB_SLOTS partial sums, one 128-byte line each, and workgroup b adds to slot b mod MB_SLOTS: eight thousand
// workgroups adding to ONE line took 99 us for 1.96 M vertices whatever else the kernel did, 12 ns a workgroup; stats sums the slots.
// Words of a slot: the four the accumulate kernel counts, in the order of the definition, then (slot 0 only) the calls whose camera block was of another
// image size.  A second set of slots, cleared by every resolve, holds the baked vertices in word 0.
constexpr u32 MB_SLOTS = 64, MB_SLOT_WORDS = 16;
constexpr u32 MB_T_USABLE = 0, MB_T_MISMATCH = 4, MB_COUNTS = 4;
constexpr u32 MB_T_BAKED_SLOTS = MB_SLOTS * MB_SLOT_WORDS, MB_T_WORDS = 2 * MB_SLOTS * MB_SLOT_WORDS;

__device__ __forceinline__ bool finite_f(float x) { return fabsf(x) < __builtin_inff(); }

__device__ __forceinline__ bool depth_agrees(float z, float d, float tolerance) { return d > 0.0f && d < __builtin_inff() && fabsf(z - d) <= tolerance; }

// Per workgroup: the lanes of each wave that hold flags[k] are counted with a ballot, the waves' counts summed by thread k, one atomic per total
template <u32 N>
__device__ __forceinline__ void add_totals(const bool (&flags)[N], u64* __restrict__ slots) {
    __shared__ u32 s_counts[N][MB_WAVES];
#pragma unroll
    for (u32 k = 0; k < N; k++) {
        const u32 n = (u32)__popcll(__ballot(flags[k]));
        if ((threadIdx.x & 63u) == 0u) s_counts[k][threadIdx.x >> 6] = n;
    }
    __syncthreads();
    if (threadIdx.x < N) {
        const u32 s = (s_counts[threadIdx.x][0] + s_counts[threadIdx.x][1]) + (s_counts[threadIdx.x][2] + s_counts[threadIdx.x][3]);
        if (s != 0u)
            (void)__hip_atomic_fetch_add(slots + (blockIdx.x % MB_SLOTS) * MB_SLOT_WORDS + threadIdx.x, (u64)s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

template <bool DEPTH, bool NORMALS>
__global__ __launch_bounds__(MB_THREADS) void bake_accumulate_kernel(const float* __restrict__ vertices, const float* __restrict__ normals, u32 V,
                                                                     const float* __restrict__ camera, const u32* __restrict__ image,
                                                                     const float* __restrict__ mesh_depth, u32 W, u32 H, float near, float depth_tolerance,
                                                                     float min_cos, u64* __restrict__ sums, u32* __restrict__ views, u64* __restrict__ totals) {
    if (!(camera[64] == (float)W && camera[65] == (float)H)) {   // (uniform: a camera block of another image size accumulates nothing)
        if (blockIdx.x == 0u && threadIdx.x == 0u) (void)__hip_atomic_fetch_add(totals + MB_T_MISMATCH, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    const u32 p = blockIdx.x * MB_THREADS + threadIdx.x;
    bool flags[MB_COUNTS] = {false, false, false, false};   // usable, in the image, visible, accumulated
    if (p < V) {
        // 1. the position: mr_vertices_kernel's arithmetic (meshraster.hip)
        const float px = vertices[3u * (size_t)p], py = vertices[3u * (size_t)p + 1u], pz = vertices[3u * (size_t)p + 2u];
        const float vx = ((camera[0] * px + camera[4] * py) + camera[8] * pz) + camera[12];
        const float vy = ((camera[1] * px + camera[5] * py) + camera[9] * pz) + camera[13];
        const float z = ((camera[2] * px + camera[6] * py) + camera[10] * pz) + camera[14];
        const float sx = (wd_div(camera[32] * vx, z) * 0.5f + 0.5f) * (float)W;
        const float sy = (wd_div((-camera[37]) * vy, z) * 0.5f + 0.5f) * (float)H;
        flags[0] = finite_f(vx) && finite_f(vy) && finite_f(z) && z >= near && finite_f(sx) && finite_f(sy) && fabsf(sx) <= 16384.0f && fabsf(sy) <= 16384.0f;
        if (flags[0]) {
            // 2. in the image (|X|, |Y| <= 2^22; the unsigned comparison is 0 <= X' <= 256 (W - 1))
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
                    for (u32 k = 0; k < 4u; k++) flags[2] = flags[2] && depth_agrees(z, d[k], depth_tolerance);
                }
                if (flags[2]) {
                    // 4. the weight
                    u32 Q = 256u;
                    if (NORMALS) {
                        const float nx = normals[3u * (size_t)p], ny = normals[3u * (size_t)p + 1u], nz = normals[3u * (size_t)p + 2u];
                        const float wx = (camera[0] * nx + camera[4] * ny) + camera[8] * nz;
                        const float wy = (camera[1] * nx + camera[5] * ny) + camera[9] * nz;
                        const float wz = (camera[2] * nx + camera[6] * ny) + camera[10] * nz;
                        const float dot = (wx * vx + wy * vy) + wz * z;
                        const float nn = (wx * wx + wy * wy) + wz * wz, vv = (vx * vx + vy * vy) + z * z;
                        const float c = wd_div(-dot, wd_sqrt(nn * vv));
                        Q = (finite_f(c) && !(c < min_cos)) ? (u32)(i32)__builtin_rintf((c > 1.0f ? 1.0f : c) * 256.0f) : 0u;
                    }
                    flags[3] = Q != 0u;
                    if (flags[3]) {
                        // 5. the sample, integers only: S <= 65536 x 255.  The colour texels are loaded here, behind the depth and the weight test: issuing
                        // them beside the depth loads measured the same time, and this form reads none for a vertex the view does not see
                        u32 texel[4];
#pragma unroll
                        for (u32 k = 0; k < 4u; k++) texel[k] = image[at[k]];
                        const u32 w[4] = {(256u - a) * (256u - b), a * (256u - b), (256u - a) * b, a * b};
                        u64 add[3];
#pragma unroll
                        for (u32 ch = 0; ch < 3u; ch++) {
                            u32 S = 0u;
#pragma unroll
                            for (u32 k = 0; k < 4u; k++) S += w[k] * ((texel[k] >> (8u * ch)) & 255u);
                            add[ch] = (u64)Q * (u64)((S + 128u) >> 8);
                        }
                        // 6. the row is this thread's alone: two 16-byte loads, two 16-byte stores
                        ulonglong2* row = reinterpret_cast<ulonglong2*>(sums + 4u * (size_t)p);
                        ulonglong2 lo = row[0], hi = row[1];
                        lo.x += add[0];
                        lo.y += add[1];
                        hi.x += add[2];
                        hi.y += (u64)Q;
                        row[0] = lo;
                        row[1] = hi;
                        const u32 n = views[p];
                        views[p] = n == 0xFFFFFFFFu ? n : n + 1u;
                    }
                }
            }
        }
    }
    add_totals(flags, totals);
}

__global__ __launch_bounds__(MB_THREADS) void bake_resolve_kernel(u32 V, const u64* __restrict__ sums, const u32* __restrict__ views, u32 min_views, u64 min_weight,
                                                                  const u32* fallback, u32* colours_out, unsigned char* __restrict__ baked_out,
                                                                  u64* __restrict__ totals) {
    const u32 p = blockIdx.x * MB_THREADS + threadIdx.x;
    bool baked = false;
    if (p < V) {
        const ulonglong2* row = reinterpret_cast<const ulonglong2*>(sums + 4u * (size_t)p);
        const ulonglong2 lo = row[0], hi = row[1];
        const u64 weight = hi.y;
        baked = views[p] >= max(min_views, 1u) && weight >= max(min_weight, (u64)1);
        u32 colour = fallback ? fallback[p] : 0u;   // (fallback may be colours_out: read before the store below)
        if (baked) {
            const u64 channel[3] = {lo.x, lo.y, hi.x};
            colour = 0xFF000000u;
#pragma unroll
            for (u32 ch = 0; ch < 3u; ch++) colour |= (u32)min((channel[ch] + 128ull * weight) / (256ull * weight), (u64)255) << (8u * ch);
        }
        colours_out[p] = colour;
        if (baked_out) baked_out[p] = baked ? 1 : 0;
    }
    const bool flags[1] = {baked};
    add_totals(flags, totals + MB_T_BAKED_SLOTS);
}

bool aligned4(const void* p) { return ((uintptr_t)p & 3u) == 0u; }

}  // namespace

// ---------------------------------------------------------------- launchers
int launch_mesh_bake_accumulate(wdgs_device* dev, const float* vertices, const float* normals, u32 V, const float* camera, const u32* image, const float* mesh_depth,
                                u32 W, u32 H, float near, float depth_tolerance, float min_cos, unsigned long long* sums, u32* views, unsigned long long* totals) {
    const dim3 grid(std::max(ceil_div(V, MB_THREADS), 1u)), block(MB_THREADS);   // (one workgroup also for no vertices: the camera block is still looked at)
#define MB_LAUNCH(D, N)                                                                                                                                    \
    WDGS_LAUNCH(dev, "mesh_bake_accumulate", (bake_accumulate_kernel<D, N>), grid, block, 0, vertices, normals, V, camera, image, mesh_depth, W, H, near, \
                depth_tolerance, min_cos, sums, views, totals)
    if (mesh_depth && normals) MB_LAUNCH(true, true);
    else if (mesh_depth) MB_LAUNCH(true, false);
    else if (normals) MB_LAUNCH(false, true);
    else MB_LAUNCH(false, false);
#undef MB_LAUNCH
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

int launch_mesh_bake_resolve(wdgs_device* dev, u32 V, const unsigned long long* sums, const u32* views, u32 min_views, unsigned long long min_weight, const u32* fallback,
                             u32* colours_out, unsigned char* baked_out, unsigned long long* totals) {
    WDGS_CHECK_HIP(hipMemsetAsync(totals + MB_T_BAKED_SLOTS, 0, sizeof(u64) * MB_SLOTS * MB_SLOT_WORDS, dev->stream));
    if (V != 0)
        WDGS_LAUNCH(dev, "mesh_bake_resolve", bake_resolve_kernel, dim3(ceil_div(V, MB_THREADS)), dim3(MB_THREADS), 0, V, sums, views, min_views, min_weight, fallback,
                    colours_out, baked_out, totals);
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

// ---------------------------------------------------------------- the C ABI object (include/webdgs.h)
struct wdgs_mesh_colour_baker {
    wdgs_device* dev = nullptr;
    DevMem<u64> sums;     // [V][4]
    DevMem<u32> views;    // [V]
    DevMem<u64> totals;   // MB_T_WORDS
    size_t capacity_v = 0;
    u32 V = 0;
    bool sized = false;
};

extern "C" int wdgs_mesh_colour_baker_create(wdgs_device* dev, wdgs_mesh_colour_baker** out) {
    WDGS_REQUIRE(dev && out, WDGS_E_INVALID, "wdgs_mesh_colour_baker_create: null argument");
    WDGS_REQUIRE(!dev->capturing, WDGS_E_STATE, "wdgs_mesh_colour_baker_create while recording a command buffer");
    auto b = std::make_unique<wdgs_mesh_colour_baker>();
    b->dev = dev;
    WDGS_TRY(b->totals.alloc(MB_T_WORDS, true, dev->stream));
    *out = b.release();
    return WDGS_OK;
}

extern "C" int wdgs_mesh_colour_baker_destroy(wdgs_mesh_colour_baker* b) {
    if (!b) return WDGS_OK;
    if (wdgs_device_alive(b->dev) && !b->dev->capturing) (void)wdgs_sync_lanes(b->dev);
    delete b;
    return WDGS_OK;
}

extern "C" int wdgs_mesh_colour_baker_reset(wdgs_mesh_colour_baker* b, uint32_t num_vertices) {
    WDGS_REQUIRE(b, WDGS_E_INVALID, "wdgs_mesh_colour_baker_reset: null argument");
    WDGS_REQUIRE(num_vertices < (1u << 31), WDGS_E_INVALID, "bakeVertexColours: %u vertices, 2^31 or more", num_vertices);
    wdgs_device* d = b->dev;
    WDGS_REQUIRE(!d->capturing, WDGS_E_STATE, "bakeVertexColours: a reset cannot be recorded into a command buffer");
    const u32 V = num_vertices;
    if (V > b->capacity_v) {
        WDGS_CHECK_HIP(wdgs_sync_lanes(d));   // (nothing in flight may still read the blocks given back)
        b->capacity_v = 0;
        b->sized = false;
        WDGS_TRY(b->sums.alloc(4 * (size_t)V, false, d->stream));
        WDGS_TRY(b->views.alloc(V, false, d->stream));
        b->capacity_v = V;
    }
    if (V != 0) {
        WDGS_CHECK_HIP(hipMemsetAsync(b->sums, 0, 32 * (size_t)V, d->stream));
        WDGS_CHECK_HIP(hipMemsetAsync(b->views, 0, 4 * (size_t)V, d->stream));
    }
    WDGS_CHECK_HIP(hipMemsetAsync(b->totals, 0, sizeof(u64) * MB_T_WORDS, d->stream));
    b->V = V;
    b->sized = true;
    return WDGS_OK;
}

extern "C" int wdgs_mesh_colour_baker_accumulate(wdgs_mesh_colour_baker* b, const void* vertices_f32_dev, const void* normals_f32_dev, uint32_t num_vertices,
                                                 const void* camera_dev, const void* image_rgba8_dev, const void* mesh_depth_f32_dev, uint32_t width, uint32_t height,
                                                 float near, float depth_tolerance, float min_cos) {
    WDGS_REQUIRE(b, WDGS_E_INVALID, "wdgs_mesh_colour_baker_accumulate: null argument");
    WDGS_REQUIRE(b->sized, WDGS_E_STATE, "bakeVertexColours: no reset precedes the accumulate");
    WDGS_REQUIRE(num_vertices == b->V, WDGS_E_STATE, "bakeVertexColours: %u vertices, the reset was for %u", num_vertices, b->V);
    WDGS_REQUIRE(width >= 1u && width <= WDGS_MESH_RASTER_MAX_SIZE && height >= 1u && height <= WDGS_MESH_RASTER_MAX_SIZE, WDGS_E_INVALID,
                 "bakeVertexColours: bad image size %ux%u (1 to %u)", width, height, WDGS_MESH_RASTER_MAX_SIZE);
    WDGS_REQUIRE(near > 0.0f && near < __builtin_inff(), WDGS_E_INVALID, "bakeVertexColours: near %g must be positive and finite", (double)near);
    WDGS_REQUIRE(depth_tolerance >= 0.0f && depth_tolerance < __builtin_inff(), WDGS_E_INVALID, "bakeVertexColours: depth tolerance %g must be finite and not negative",
                 (double)depth_tolerance);
    WDGS_REQUIRE(min_cos >= 0.0f && min_cos <= 1.0f, WDGS_E_INVALID, "bakeVertexColours: min_cos %g is not in [0, 1]", (double)min_cos);
    WDGS_REQUIRE(camera_dev && image_rgba8_dev && (num_vertices == 0 || vertices_f32_dev), WDGS_E_INVALID, "wdgs_mesh_colour_baker_accumulate: null vertices, camera or image");
    WDGS_REQUIRE(aligned4(vertices_f32_dev) && aligned4(normals_f32_dev) && aligned4(camera_dev) && aligned4(image_rgba8_dev) && aligned4(mesh_depth_f32_dev), WDGS_E_INVALID,
                 "wdgs_mesh_colour_baker_accumulate: misaligned buffer");
    return launch_mesh_bake_accumulate(b->dev, static_cast<const float*>(vertices_f32_dev), static_cast<const float*>(normals_f32_dev), num_vertices,
                                       static_cast<const float*>(camera_dev), static_cast<const u32*>(image_rgba8_dev), static_cast<const float*>(mesh_depth_f32_dev), width,
                                       height, near, depth_tolerance, min_cos, b->sums, b->views, b->totals);
}

extern "C" int wdgs_mesh_colour_baker_resolve(wdgs_mesh_colour_baker* b, void* colours_out_rgba8_dev, const void* fallback_rgba8_dev, void* baked_out_u8_dev,
                                              uint32_t num_vertices, uint32_t min_views, uint64_t min_weight) {
    WDGS_REQUIRE(b, WDGS_E_INVALID, "wdgs_mesh_colour_baker_resolve: null argument");
    WDGS_REQUIRE(b->sized, WDGS_E_STATE, "bakeVertexColours: no reset precedes the resolve");
    WDGS_REQUIRE(num_vertices == b->V, WDGS_E_STATE, "bakeVertexColours: %u vertices, the reset was for %u", num_vertices, b->V);
    WDGS_REQUIRE(num_vertices == 0 || colours_out_rgba8_dev, WDGS_E_INVALID, "wdgs_mesh_colour_baker_resolve: null colours output");
    WDGS_REQUIRE(aligned4(colours_out_rgba8_dev) && aligned4(fallback_rgba8_dev), WDGS_E_INVALID, "wdgs_mesh_colour_baker_resolve: misaligned colours");
    return launch_mesh_bake_resolve(b->dev, num_vertices, b->sums, b->views, min_views, min_weight, static_cast<const u32*>(fallback_rgba8_dev),
                                    static_cast<u32*>(colours_out_rgba8_dev), static_cast<unsigned char*>(baked_out_u8_dev), b->totals);
}

extern "C" int wdgs_mesh_colour_baker_read(wdgs_mesh_colour_baker* b, uint64_t* sums_out, uint32_t* views_out) {
    WDGS_REQUIRE(b, WDGS_E_INVALID, "wdgs_mesh_colour_baker_read: null argument");
    WDGS_REQUIRE(b->sized, WDGS_E_STATE, "bakeVertexColours: no reset precedes the read");
    wdgs_device* d = b->dev;
    WDGS_REQUIRE(!d->capturing, WDGS_E_STATE, "bakeVertexColours: the read of the state waits and cannot be recorded into a command buffer");
    if (b->V != 0 && sums_out) WDGS_CHECK_HIP(hipMemcpyAsync(sums_out, b->sums, 32 * (size_t)b->V, hipMemcpyDeviceToHost, d->stream));
    if (b->V != 0 && views_out) WDGS_CHECK_HIP(hipMemcpyAsync(views_out, b->views, 4 * (size_t)b->V, hipMemcpyDeviceToHost, d->stream));
    WDGS_CHECK_HIP(wdgs_sync_lanes(d));
    return WDGS_OK;
}

extern "C" int wdgs_mesh_colour_baker_stats(wdgs_mesh_colour_baker* b, uint64_t* usable, uint64_t* in_image, uint64_t* visible, uint64_t* accumulated,
                                            uint64_t* viewport_mismatch, uint64_t* baked_vertices) {
    WDGS_REQUIRE(b, WDGS_E_INVALID, "wdgs_mesh_colour_baker_stats: null argument");
    WDGS_REQUIRE(b->sized, WDGS_E_STATE, "bakeVertexColours: no reset precedes the read of its statistics");
    wdgs_device* d = b->dev;
    WDGS_REQUIRE(!d->capturing, WDGS_E_STATE, "bakeVertexColours: the read of the statistics waits and cannot be recorded into a command buffer");
    std::vector<u64> host(MB_T_WORDS);
    WDGS_CHECK_HIP(hipMemcpyAsync(host.data(), b->totals, sizeof(u64) * MB_T_WORDS, hipMemcpyDeviceToHost, d->stream));
    WDGS_CHECK_HIP(wdgs_sync_lanes(d));
    uint64_t* const outs[MB_COUNTS + 2] = {usable, in_image, visible, accumulated, viewport_mismatch, baked_vertices};
    for (u32 k = 0; k < MB_COUNTS + 2; k++) {   // (the slots of a total summed; the last one from the resolve's set)
        const u32 word = k <= MB_T_MISMATCH ? k : MB_T_BAKED_SLOTS;
        u64 sum = 0;
        for (u32 s = 0; s < MB_SLOTS; s++) sum += host[word + s * MB_SLOT_WORDS];
        if (outs[k]) *outs[k] = sum;
    }
    return WDGS_OK;
}
