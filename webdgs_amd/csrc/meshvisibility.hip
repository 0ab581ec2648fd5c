// Per-face visibility over views, the rule on its counters and a face filter that compacts by any mask (no counterpart in the reference,
// which renders splats only).  include/webdgs.h states the definitions operation by operation; tests/meshvisibility_ref.py restates them.
//
// The accumulator takes the face image the mesh rasterizer writes (and, optionally, the mesh's and the model's depth images of the same view) and adds, per
// face, the pixels that show it, those of them whose two depths agree, and -- once per call -- one view.  Everything is integer work: the pixel and agreeing
// counts of a face live in the two halves of one u64 word and receive ONE 64-bit add per run of equal face indices within a wave (the refusal of a call that
// could carry the low half into the high one is host arithmetic); the view count comes from a per-face stamp word exchanged with the number of the current
// view, which exactly one exchanger finds older.  Sums and exchanges do not depend on the order of their operands, so every byte is a function of the inputs.
//
// Section 16's to 20's rule holds: no spin-wait, no inter-workgroup flag, no look-back, no grid barrier, no float atomics; what one launch writes the next one
// reads, and visibility comes from launch boundaries only.  The one word a kernel reads that others of the same launch write is the stamp, in a relaxed load in
// front of the exchange; section 21 holds the argument that skipping the exchange is exact for any value that load may return.
//
// The filter is meshclean.hip's compaction under a mask that need not follow components: flags, the library's scan, and meshclean's emit launcher.
#include <algorithm>
#include <memory>

#include "launch.h"

namespace {

typedef unsigned long long u64;

constexpr u32 FV_THREADS = 256;
constexpr u32 FV_WAVES = FV_THREADS / 64;
constexpr u32 FV_LANE_PIXELS = 4;                      // one 16-byte load per image and lane
constexpr u32 FV_CHUNK = 64 * FV_LANE_PIXELS;          // the pixels a wave takes at once
constexpr u32 FV_ITEMS = 4;                            // consecutive chunks per wave: a run is carried from one to the next
constexpr u32 FV_EMPTY = 0xFFFFFFFFu;
// The state block, u64 words: the views accumulated (the number of the current view is one more), the foreign, counted and agreeing pixels
// (words 1, 2, 3, in the order the kernel sums them)
constexpr u32 FV_S_VIEWS = 0, FV_S_FOREIGN = 1, FV_S_WORDS = 4;

__device__ __forceinline__ bool depth_present(float d) { return d > 0.0f && d < __builtin_inff(); }   // (meshraster.hip's rule for wdgs_depth_agreement)

struct FvTables {
    u64* pairs;    // [F]: pixels in the low half, agreeing in the high half
    u32* stamps;   // [F]: the number of the last view that showed the face; 0: none yet
    u32* views;    // [F]
};

// One run of `px` pixels of face f, `ag` of them agreeing.  The stamp: whoever exchanges finds either an older number -- exactly one does, the first in the
// word's modification order -- or the current one; a load that already returns the current number can only be followed by exchanges that find it too.
__device__ __forceinline__ void fv_add(const FvTables& t, u32 view, u32 f, u32 px, u32 ag) {
    if (f == FV_EMPTY) return;
    (void)__hip_atomic_fetch_add(t.pairs + f, (u64)px | ((u64)ag << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (__hip_atomic_load(t.stamps + f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != view) {
        if (__hip_atomic_exchange(t.stamps + f, view, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != view)
            (void)__hip_atomic_fetch_add(t.views + f, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__device__ __forceinline__ u32 fv_wave_sum(u32 x) {
#pragma unroll
    for (u32 d = 32; d >= 1; d >>= 1) x += (u32)__shfl_xor((int)x, (int)d, 64);
    return x;
}

// The image is taken as one row of npix pixels; a wave owns FV_ITEMS consecutive chunks of FV_CHUNK pixels, lane l of a chunk its pixels 4 l .. 4 l + 3.
// Per chunk every lane cuts its four pixels into segments of equal key (the face index; FV_EMPTY for an empty, a foreign and a past-the-end pixel): a HEAD
// segment from its first pixel on, and, unless all four are equal (a UNIFORM lane), a TAIL segment up to its last and at most two pixels between them, which
// are runs of their own and added at once.  A run of the chunk is then a tail, or a head that does not continue the lane before it, followed by the heads of
// the lanes after it for as long as they continue it and were uniform up to there; two ballots (the lanes whose head continues, the lanes that are not uniform)
// give every run's leader the mask of its members, and six more -- the bits of the members' pixel and agreeing counts, each at most 4 -- its sums.  One add
// per run; the run that holds the chunk's last pixel is withheld and carried, in wave-uniform registers, into the next chunk, whose lane 0 joins it or adds it.
// Every lane runs every ballot and shuffle; the loop's exits are uniform.
template <bool DEPTH>
__global__ __launch_bounds__(FV_THREADS) void fv_accumulate_kernel(const u32* __restrict__ face_image, const float* __restrict__ mesh_depth,
                                                                   const float* __restrict__ model_depth, const float* __restrict__ weight_sum, float min_weight_sum,
                                                                   float threshold, u32 npix, u32 F, FvTables t, u64* __restrict__ state) {
    __shared__ u32 s_sums[3][FV_WAVES];
    const u32 lane = threadIdx.x & 63u;
    const u32 wave = (u32)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * FV_WAVES + (threadIdx.x >> 6)));
    const u32 view = (u32)state[FV_S_VIEWS] + 1u;   // (written by the launch after this one only)
    u32 carry_key = FV_EMPTY, carry_px = 0u, carry_ag = 0u;
    u32 n_foreign = 0u, n_counted = 0u, n_agreeing = 0u;
    for (u32 item = 0; item < FV_ITEMS; item++) {
        const u64 base = ((u64)wave * FV_ITEMS + item) * FV_CHUNK;
        if (base >= (u64)npix) break;
        const u32 p0 = (u32)base + lane * FV_LANE_PIXELS;
        u32 key[FV_LANE_PIXELS], agree[FV_LANE_PIXELS];
        if (p0 + FV_LANE_PIXELS <= npix) {
            const uint4 q = *reinterpret_cast<const uint4*>(face_image + p0);
            key[0] = q.x; key[1] = q.y; key[2] = q.z; key[3] = q.w;
            if (DEPTH) {
                const float4 a = *reinterpret_cast<const float4*>(mesh_depth + p0), b = *reinterpret_cast<const float4*>(model_depth + p0);
                float4 w = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (weight_sum) w = *reinterpret_cast<const float4*>(weight_sum + p0);
                const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w}, wv[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
                for (u32 j = 0; j < FV_LANE_PIXELS; j++) {
                    const bool has_a = depth_present(av[j]), has_b = depth_present(bv[j]) && (!weight_sum || wv[j] >= min_weight_sum);
                    agree[j] = (has_a && has_b && fabsf(av[j] - bv[j]) <= threshold) ? 1u : 0u;
                }
            }
        } else {
#pragma unroll
            for (u32 j = 0; j < FV_LANE_PIXELS; j++) {
                const u32 p = p0 + j;
                key[j] = FV_EMPTY;
                agree[j] = 0u;
                if (p < npix) {
                    key[j] = face_image[p];
                    if (DEPTH) {
                        const float a = mesh_depth[p], b = model_depth[p];
                        const bool has_a = depth_present(a), has_b = depth_present(b) && (!weight_sum || weight_sum[p] >= min_weight_sum);
                        agree[j] = (has_a && has_b && fabsf(a - b) <= threshold) ? 1u : 0u;
                    }
                }
            }
        }
#pragma unroll
        for (u32 j = 0; j < FV_LANE_PIXELS; j++) {
            if (!DEPTH) agree[j] = 1u;
            if (key[j] >= F) {   // empty or foreign: no address is formed from it
                if (key[j] != FV_EMPTY) n_foreign++;
                key[j] = FV_EMPTY;
                agree[j] = 0u;
            } else {
                n_counted++;
                n_agreeing += agree[j];
            }
        }
        // the lane's segments
        const u32 hk = key[0], tk = key[3];
        u32 h = 1u, ha = agree[0], tl = 1u, ta = agree[3];
        bool same = true;
#pragma unroll
        for (u32 j = 1; j < FV_LANE_PIXELS; j++) {
            same = same && key[j] == hk;
            if (same) { h++; ha += agree[j]; }
        }
        const bool uniform = h == FV_LANE_PIXELS;
        same = true;
#pragma unroll
        for (u32 j = 1; j < FV_LANE_PIXELS; j++) {
            same = same && key[FV_LANE_PIXELS - 1u - j] == tk;
            if (same) { tl++; ta += agree[FV_LANE_PIXELS - 1u - j]; }
        }
        if (!uniform) {   // pixels 1 and 2 where neither the head nor the tail holds them
            const u32 m0 = h, m1 = FV_LANE_PIXELS - tl;
            if (m0 == 1u && m1 == 3u && key[1] == key[2]) {
                fv_add(t, view, key[1], 2u, agree[1] + agree[2]);
            } else {
                if (m0 <= 1u && 1u < m1) fv_add(t, view, key[1], 1u, agree[1]);
                if (m0 <= 2u && 2u < m1) fv_add(t, view, key[2], 1u, agree[2]);
            }
        }
        // the carried run meets lane 0's head
        const u32 prev_tk = (u32)__shfl_up((int)tk, 1u, 64);
        const bool starts = lane == 0u || prev_tk != hk;   // the head does not continue the lane before
        const bool joins_carry = carry_key == (u32)__shfl((int)hk, 0, 64);
        u32 h_px = h, h_ag = ha;
        if (lane == 0u) {
            if (joins_carry) { h_px += carry_px; h_ag += carry_ag; }
            else fv_add(t, view, carry_key, carry_px, carry_ag);
        }
        if (!uniform && starts) fv_add(t, view, hk, h_px, h_ag);   // a head that is a run by itself
        // the runs that reach over lanes
        const u64 not_uniform = __ballot(!uniform), continues = __ballot(!starts);
        const u64 above = lane == 63u ? 0ull : (~0ull << (lane + 1u));
        const u64 stop_before = ~continues & above, stop_at = not_uniform & above;
        const u32 x = stop_before ? (u32)(__ffsll((long long)stop_before) - 1) : 64u;
        const u32 y = stop_at ? (u32)__ffsll((long long)stop_at) : 65u;   // (one past the first lane above that is not uniform)
        const u32 end = min(x, y);
        const u64 members = above & (end >= 64u ? ~0ull : ((1ull << end) - 1ull));
        const bool leader = !uniform || starts;
        u32 px = uniform ? h_px : tl, ag = uniform ? h_ag : ta;
#pragma unroll
        for (u32 b = 0; b < 3u; b++) {
            px += (u32)__popcll(__ballot(((h >> b) & 1u) != 0u) & members) << b;
            ag += (u32)__popcll(__ballot(((ha >> b) & 1u) != 0u) & members) << b;
        }
        const bool last = leader && (lane == 63u || (end == 64u && (not_uniform >> 63) == 0ull));
        if (leader && !last) fv_add(t, view, tk, px, ag);
        const int src = __ffsll((long long)__ballot(last)) - 1;   // exactly one lane
        carry_key = (u32)__shfl((int)tk, src, 64);
        carry_px = (u32)__shfl((int)px, src, 64);
        carry_ag = (u32)__shfl((int)ag, src, 64);
    }
    if (lane == 0u) fv_add(t, view, carry_key, carry_px, carry_ag);
    n_foreign = fv_wave_sum(n_foreign);
    n_counted = fv_wave_sum(n_counted);
    n_agreeing = fv_wave_sum(n_agreeing);
    if (lane == 0u) {
        s_sums[0][threadIdx.x >> 6] = n_foreign;
        s_sums[1][threadIdx.x >> 6] = n_counted;
        s_sums[2][threadIdx.x >> 6] = n_agreeing;
    }
    __syncthreads();
    if (threadIdx.x < 3u) {
        const u32 s = (s_sums[threadIdx.x][0] + s_sums[threadIdx.x][1]) + (s_sums[threadIdx.x][2] + s_sums[threadIdx.x][3]);
        if (s != 0u) (void)__hip_atomic_fetch_add(state + FV_S_FOREIGN + threadIdx.x, (u64)s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// The view is over: the next accumulate stamps with the next number.  A launch of its own, so that a recorded accumulate counts its views when replayed
__global__ void fv_advance_kernel(u64* __restrict__ state) { state[FV_S_VIEWS] += 1ull; }

// counters u32[F][3] = { pixels, agreeing, views }
__global__ __launch_bounds__(FV_THREADS) void fv_pack_kernel(u32 F, const u64* __restrict__ pairs, const u32* __restrict__ views, u32* __restrict__ counters) {
    const u32 f = blockIdx.x * FV_THREADS + threadIdx.x;
    if (f >= F) return;
    const u64 w = pairs[f];
    counters[3u * (size_t)f] = (u32)w;
    counters[3u * (size_t)f + 1u] = (u32)(w >> 32);
    counters[3u * (size_t)f + 2u] = views[f];
}

__global__ __launch_bounds__(FV_THREADS) void fv_flags_kernel(u32 F, const u32* __restrict__ counters, u32 min_pixels, u32 min_views, u32 min_agreeing, u32 min_agreeing_q16,
                                                              unsigned char* __restrict__ keep) {
    const u32 f = blockIdx.x * FV_THREADS + threadIdx.x;
    if (f >= F) return;
    const u32 pixels = counters[3u * (size_t)f], agreeing = counters[3u * (size_t)f + 1u], views = counters[3u * (size_t)f + 2u];
    const bool k = pixels >= min_pixels && views >= min_views && agreeing >= min_agreeing && (u64)agreeing * 65536ull >= (u64)min_agreeing_q16 * (u64)pixels;
    keep[f] = k ? 1 : 0;
}

// One thread per face: face_flags[f] = 1 for a face whose flag is set and whose indices are vertices, whose three vertices are marked (equal stores into a
// cleared array); the invalid faces, flagged or not, are counted, one atomic per wave
__global__ __launch_bounds__(FV_THREADS) void ff_flags_kernel(const u32* __restrict__ faces, u32 F, u32 V, const unsigned char* __restrict__ keep, u32* __restrict__ face_flags,
                                                              u32* __restrict__ vertex_flags, u32* __restrict__ invalid_faces) {
    const u32 f = blockIdx.x * FV_THREADS + threadIdx.x;
    bool invalid = false;
    if (f < F) {
        const u32 a = faces[3u * (size_t)f], b = faces[3u * (size_t)f + 1u], c = faces[3u * (size_t)f + 2u];
        invalid = !(a < V && b < V && c < V);
        const bool kept = !invalid && keep[f] != 0;
        face_flags[f] = kept ? 1u : 0u;
        if (kept) {
            vertex_flags[a] = 1u;
            vertex_flags[b] = 1u;
            vertex_flags[c] = 1u;
        }
    }
    const u64 m = __ballot(invalid);
    if (m != 0ull && (threadIdx.x & 63u) == (u32)(__ffsll((long long)m) - 1)) atomicAdd(invalid_faces, (u32)__popcll(m));
}

bool positive_finite(float x) { return x > 0.0f && x < __builtin_inff(); }

}  // namespace

// ---------------------------------------------------------------- launchers
int launch_face_visibility_accumulate(wdgs_device* dev, const u32* face_image, const float* mesh_depth, const float* model_depth, const float* weight_sum,
                                      float min_weight_sum, float threshold, u32 npix, u32 F, unsigned long long* pairs, u32* stamps, u32* views,
                                      unsigned long long* state) {
    const u32 waves = ceil_div(npix, FV_CHUNK * FV_ITEMS);
    const dim3 grid(ceil_div(waves, FV_WAVES));
    const FvTables t{pairs, stamps, views};
    if (mesh_depth)
        WDGS_LAUNCH(dev, "face_visibility_accumulate", fv_accumulate_kernel<true>, grid, dim3(FV_THREADS), 0, face_image, mesh_depth, model_depth, weight_sum, min_weight_sum,
                    threshold, npix, F, t, state);
    else
        WDGS_LAUNCH(dev, "face_visibility_accumulate", fv_accumulate_kernel<false>, grid, dim3(FV_THREADS), 0, face_image, mesh_depth, model_depth, weight_sum, min_weight_sum,
                    threshold, npix, F, t, state);
    WDGS_LAUNCH(dev, "face_visibility_advance", fv_advance_kernel, dim3(1), dim3(1), 0, state);
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

int launch_face_visibility_pack(wdgs_device* dev, u32 F, const unsigned long long* pairs, const u32* views, u32* counters) {
    if (F == 0) return WDGS_OK;
    WDGS_LAUNCH(dev, "face_visibility_pack", fv_pack_kernel, dim3(ceil_div(F, FV_THREADS)), dim3(FV_THREADS), 0, F, pairs, views, counters);
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

int launch_face_visibility_flags(wdgs_device* dev, u32 F, const u32* counters, u32 min_pixels, u32 min_views, u32 min_agreeing, u32 min_agreeing_q16, unsigned char* keep) {
    if (F == 0) return WDGS_OK;
    WDGS_LAUNCH(dev, "face_visibility_flags", fv_flags_kernel, dim3(ceil_div(F, FV_THREADS)), dim3(FV_THREADS), 0, F, counters, min_pixels, min_views, min_agreeing,
                min_agreeing_q16, keep);
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

int launch_face_filter_flags(wdgs_device* dev, const u32* faces, u32 F, u32 V, const unsigned char* keep, u32* face_flags, u32* vertex_flags, u32* invalid_faces) {
    WDGS_CHECK_HIP(hipMemsetAsync(invalid_faces, 0, 4, dev->stream));
    if (V != 0) WDGS_CHECK_HIP(hipMemsetAsync(vertex_flags, 0, 4 * (size_t)V, dev->stream));
    if (F != 0) WDGS_LAUNCH(dev, "face_filter_flags", ff_flags_kernel, dim3(ceil_div(F, FV_THREADS)), dim3(FV_THREADS), 0, faces, F, V, keep, face_flags, vertex_flags, invalid_faces);
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

// ---------------------------------------------------------------- the C ABI objects (include/webdgs.h)
struct wdgs_face_visibility {
    wdgs_device* dev = nullptr;
    DevMem<u64> pairs;               // [F]
    DevMem<u32> stamps, views;       // [F]
    DevMem<u32> counters;            // [3 F]: what get hands out
    DevMem<u64> state;               // FV_S_WORDS
    size_t capacity_f = 0;
    u32 F = 0;
    bool sized = false;
    u64 host_views = 0;              // the accumulates enqueued or recorded since the reset: what the capacity check counts
};

extern "C" int wdgs_face_visibility_create(wdgs_device* dev, wdgs_face_visibility** out) {
    WDGS_REQUIRE(dev && out, WDGS_E_INVALID, "wdgs_face_visibility_create: null argument");
    WDGS_REQUIRE(!dev->capturing, WDGS_E_STATE, "wdgs_face_visibility_create while recording a command buffer");
    auto v = std::make_unique<wdgs_face_visibility>();
    v->dev = dev;
    WDGS_TRY(v->state.alloc(FV_S_WORDS, true, dev->stream));
    *out = v.release();
    return WDGS_OK;
}

extern "C" int wdgs_face_visibility_destroy(wdgs_face_visibility* v) {
    if (!v) return WDGS_OK;
    if (wdgs_device_alive(v->dev) && !v->dev->capturing) (void)wdgs_sync_lanes(v->dev);
    delete v;
    return WDGS_OK;
}

extern "C" int wdgs_face_visibility_reset(wdgs_face_visibility* v, uint32_t num_faces) {
    WDGS_REQUIRE(v, WDGS_E_INVALID, "wdgs_face_visibility_reset: null argument");
    WDGS_REQUIRE(num_faces < (1u << 31), WDGS_E_INVALID, "faceVisibility: %u faces, 2^31 or more", num_faces);
    wdgs_device* d = v->dev;
    const u32 F = num_faces;
    if (F > v->capacity_f) {
        WDGS_REQUIRE(!d->capturing, WDGS_E_STATE, "faceVisibility: the object's arrays have to grow, which cannot be recorded into a command buffer (reset once before recording)");
        WDGS_CHECK_HIP(wdgs_sync_lanes(d));   // (nothing in flight may still read the blocks given back)
        v->capacity_f = 0;
        v->sized = false;
        WDGS_TRY(v->pairs.alloc(F, false, d->stream));
        WDGS_TRY(v->stamps.alloc(F, false, d->stream));
        WDGS_TRY(v->views.alloc(F, false, d->stream));
        WDGS_TRY(v->counters.alloc(3 * (size_t)F, false, d->stream));
        v->capacity_f = F;
    }
    if (F != 0) {
        WDGS_CHECK_HIP(hipMemsetAsync(v->pairs, 0, 8 * (size_t)F, d->stream));
        WDGS_CHECK_HIP(hipMemsetAsync(v->stamps, 0, 4 * (size_t)F, d->stream));
        WDGS_CHECK_HIP(hipMemsetAsync(v->views, 0, 4 * (size_t)F, d->stream));
        WDGS_CHECK_HIP(hipMemsetAsync(v->counters, 0, 12 * (size_t)F, d->stream));
    }
    WDGS_CHECK_HIP(hipMemsetAsync(v->state, 0, sizeof(u64) * FV_S_WORDS, d->stream));
    v->F = F;
    v->host_views = 0;
    v->sized = true;
    return WDGS_OK;
}

extern "C" int wdgs_face_visibility_accumulate(wdgs_face_visibility* v, const void* face_image_u32_dev, const void* mesh_depth_f32_dev, const void* model_depth_f32_dev,
                                               const void* model_weight_sum_f32_dev, float min_weight_sum, float threshold, uint32_t width, uint32_t height) {
    WDGS_REQUIRE(v, WDGS_E_INVALID, "wdgs_face_visibility_accumulate: null argument");
    WDGS_REQUIRE(v->sized, WDGS_E_STATE, "faceVisibility: no reset precedes the accumulate");
    WDGS_REQUIRE(width >= 1u && width <= WDGS_MESH_RASTER_MAX_SIZE && height >= 1u && height <= WDGS_MESH_RASTER_MAX_SIZE, WDGS_E_INVALID,
                 "faceVisibility: bad image size %ux%u (1 to %u)", width, height, WDGS_MESH_RASTER_MAX_SIZE);
    WDGS_REQUIRE(positive_finite(threshold), WDGS_E_INVALID, "faceVisibility: threshold %g must be positive and finite", (double)threshold);
    WDGS_REQUIRE((mesh_depth_f32_dev == nullptr) == (model_depth_f32_dev == nullptr), WDGS_E_INVALID, "faceVisibility: the mesh's and the model's depth image come together or not at all");
    WDGS_REQUIRE(model_depth_f32_dev || !model_weight_sum_f32_dev, WDGS_E_INVALID, "faceVisibility: a weight sum needs the depth images");
    const u64 npix = (u64)width * height;
    WDGS_REQUIRE((v->host_views + 1ull) * npix < (1ull << 32), WDGS_E_CAPACITY, "faceVisibility: view %llu of %ux%u pixels could overflow a 32-bit pixel count (reset, or read and start anew)",
                 (unsigned long long)(v->host_views + 1ull), width, height);
    WDGS_REQUIRE(face_image_u32_dev, WDGS_E_INVALID, "wdgs_face_visibility_accumulate: null face image");
    WDGS_REQUIRE((((uintptr_t)face_image_u32_dev | (uintptr_t)mesh_depth_f32_dev | (uintptr_t)model_depth_f32_dev | (uintptr_t)model_weight_sum_f32_dev) & 15u) == 0u,
                 WDGS_E_INVALID, "wdgs_face_visibility_accumulate: misaligned image (16 bytes)");
    WDGS_TRY(launch_face_visibility_accumulate(v->dev, static_cast<const u32*>(face_image_u32_dev), static_cast<const float*>(mesh_depth_f32_dev),
                                               static_cast<const float*>(model_depth_f32_dev), static_cast<const float*>(model_weight_sum_f32_dev), min_weight_sum, threshold,
                                               (u32)npix, v->F, v->pairs, v->stamps, v->views, v->state));
    v->host_views += 1ull;
    return WDGS_OK;
}

extern "C" int wdgs_face_visibility_get(wdgs_face_visibility* v, void** counters_u32_dev) {
    WDGS_REQUIRE(v && counters_u32_dev, WDGS_E_INVALID, "wdgs_face_visibility_get: null argument");
    WDGS_REQUIRE(v->sized, WDGS_E_STATE, "faceVisibility: no reset precedes the read");
    WDGS_TRY(launch_face_visibility_pack(v->dev, v->F, v->pairs, v->views, v->counters));
    *counters_u32_dev = v->F ? v->counters.get() : nullptr;
    return WDGS_OK;
}

extern "C" int wdgs_face_visibility_stats(wdgs_face_visibility* v, uint64_t* views, uint64_t* foreign_pixels, uint64_t* counted_pixels, uint64_t* agreeing_pixels) {
    WDGS_REQUIRE(v, WDGS_E_INVALID, "wdgs_face_visibility_stats: null argument");
    WDGS_REQUIRE(v->sized, WDGS_E_STATE, "faceVisibility: no reset precedes the read of its statistics");
    wdgs_device* d = v->dev;
    WDGS_REQUIRE(!d->capturing, WDGS_E_STATE, "faceVisibility: the read of the statistics waits and cannot be recorded into a command buffer");
    u64 host[FV_S_WORDS];
    WDGS_CHECK_HIP(hipMemcpyAsync(host, v->state, sizeof(host), hipMemcpyDeviceToHost, d->stream));
    WDGS_CHECK_HIP(wdgs_sync_lanes(d));
    v->host_views = std::max<u64>(v->host_views, host[FV_S_VIEWS]);   // (replays of a recorded accumulate are views the host has not counted)
    uint64_t* const outs[FV_S_WORDS] = {views, foreign_pixels, counted_pixels, agreeing_pixels};
    for (u32 k = 0; k < FV_S_WORDS; k++) {
        if (outs[k]) *outs[k] = host[k];
    }
    return WDGS_OK;
}

extern "C" int wdgs_face_visibility_flags(wdgs_device* dev, const void* counters_u32_dev, uint32_t num_faces, uint32_t min_pixels, uint32_t min_views, uint32_t min_agreeing,
                                          uint32_t min_agreeing_q16, void* keep_u8_dev) {
    WDGS_REQUIRE(dev, WDGS_E_INVALID, "wdgs_face_visibility_flags: null argument");
    WDGS_REQUIRE(num_faces < (1u << 31), WDGS_E_INVALID, "faceVisibility: %u faces, 2^31 or more", num_faces);
    WDGS_REQUIRE(min_agreeing_q16 <= 65536u, WDGS_E_INVALID, "faceVisibility: an agreeing fraction of %u / 65536 is more than 1", min_agreeing_q16);
    WDGS_REQUIRE(num_faces == 0 || (counters_u32_dev && keep_u8_dev), WDGS_E_INVALID, "wdgs_face_visibility_flags: null counters or flags");
    WDGS_REQUIRE(((uintptr_t)counters_u32_dev & 3u) == 0u, WDGS_E_INVALID, "wdgs_face_visibility_flags: misaligned counters");
    return launch_face_visibility_flags(dev, num_faces, static_cast<const u32*>(counters_u32_dev), min_pixels, min_views, min_agreeing, min_agreeing_q16,
                                        static_cast<unsigned char*>(keep_u8_dev));
}

struct wdgs_mesh_face_filter {
    wdgs_device* dev = nullptr;
    DevMem<u32> vertex_flags, vertex_offsets;   // [V]
    DevMem<u32> face_flags, face_offsets;       // [F]
    DevMem<u32> counters;                       // kept vertices, kept faces, invalid faces
    ScanScratch scan;
    u32 capacity_v = 0, capacity_f = 0, capacity_scan = 0;
    bool selected = false;
    const void* faces = nullptr;                // the caller's, read again by compact
    u32 V = 0, F = 0, kept_v = 0, kept_f = 0;
};

extern "C" int wdgs_mesh_face_filter_create(wdgs_device* dev, wdgs_mesh_face_filter** out) {
    WDGS_REQUIRE(dev && out, WDGS_E_INVALID, "wdgs_mesh_face_filter_create: null argument");
    WDGS_REQUIRE(!dev->capturing, WDGS_E_STATE, "wdgs_mesh_face_filter_create while recording a command buffer");
    auto c = std::make_unique<wdgs_mesh_face_filter>();
    c->dev = dev;
    WDGS_TRY(c->counters.alloc(4, true, dev->stream));
    *out = c.release();
    return WDGS_OK;
}

extern "C" int wdgs_mesh_face_filter_destroy(wdgs_mesh_face_filter* c) {
    if (!c) return WDGS_OK;
    if (wdgs_device_alive(c->dev) && !c->dev->capturing) (void)wdgs_sync_lanes(c->dev);
    delete c;
    return WDGS_OK;
}

extern "C" int wdgs_mesh_face_filter_select(wdgs_mesh_face_filter* c, const void* faces_u32_dev, uint32_t num_faces, uint32_t num_vertices, const void* keep_u8_dev,
                                            uint32_t* kept_vertices, uint32_t* kept_faces, uint32_t* invalid_faces) {
    WDGS_REQUIRE(c && kept_vertices && kept_faces && invalid_faces, WDGS_E_INVALID, "wdgs_mesh_face_filter_select: null argument");
    c->selected = false;   // (a refused selection leaves nothing to compact)
    WDGS_REQUIRE(num_faces == 0 || (faces_u32_dev && keep_u8_dev), WDGS_E_INVALID, "wdgs_mesh_face_filter_select: null faces or flags");
    WDGS_REQUIRE(num_faces < (1u << 31) && num_vertices < (1u << 31), WDGS_E_INVALID, "filterFaces: %u faces over %u vertices, 2^31 or more", num_faces, num_vertices);
    WDGS_REQUIRE(((uintptr_t)faces_u32_dev & 3u) == 0u, WDGS_E_INVALID, "wdgs_mesh_face_filter_select: misaligned faces");
    wdgs_device* d = c->dev;
    WDGS_REQUIRE(!d->capturing, WDGS_E_STATE, "filterFaces: the selection waits for its counts and cannot be recorded into a command buffer");
    *kept_vertices = *kept_faces = *invalid_faces = 0;
    const u32 V = num_vertices, F = num_faces;
    if (V > c->capacity_v || F > c->capacity_f || std::max(V, F) > c->capacity_scan) {
        WDGS_CHECK_HIP(wdgs_sync_lanes(d));   // (nothing in flight may still read the blocks given back)
        if (V > c->capacity_v) {
            c->capacity_v = 0;
            WDGS_TRY(c->vertex_flags.alloc(V, false, d->stream));
            WDGS_TRY(c->vertex_offsets.alloc(V, false, d->stream));
            c->capacity_v = V;
        }
        if (F > c->capacity_f) {
            c->capacity_f = 0;
            WDGS_TRY(c->face_flags.alloc(F, false, d->stream));
            WDGS_TRY(c->face_offsets.alloc(F, false, d->stream));
            c->capacity_f = F;
        }
        if (std::max(V, F) > c->capacity_scan) {
            c->capacity_scan = 0;
            WDGS_TRY(scan_scratch_create(&c->scan, std::max(V, F)));
            c->capacity_scan = std::max(V, F);
        }
    }
    WDGS_CHECK_HIP(hipMemsetAsync(c->counters, 0, 16, d->stream));
    WDGS_TRY(launch_face_filter_flags(d, static_cast<const u32*>(faces_u32_dev), F, V, static_cast<const unsigned char*>(keep_u8_dev), c->face_flags, c->vertex_flags,
                                      c->counters + 2));
    WDGS_TRY(scan_exclusive_u32(d, &c->scan, c->vertex_flags, c->vertex_offsets, V, c->counters));
    WDGS_TRY(scan_exclusive_u32(d, &c->scan, c->face_flags, c->face_offsets, F, c->counters + 1));
    u32 host[3] = {0u, 0u, 0u};
    WDGS_CHECK_HIP(hipMemcpyAsync(host, c->counters, sizeof(host), hipMemcpyDeviceToHost, d->stream));
    WDGS_CHECK_HIP(wdgs_sync_lanes(d));
    c->faces = faces_u32_dev;
    c->V = V;
    c->F = F;
    c->kept_v = host[0];
    c->kept_f = host[1];
    c->selected = true;
    *kept_vertices = host[0];
    *kept_faces = host[1];
    *invalid_faces = host[2];
    return WDGS_OK;
}

extern "C" int wdgs_mesh_face_filter_compact(wdgs_mesh_face_filter* c, const void* vertices_f32_dev, void* vertices_out_f32_dev, void* faces_out_u32_dev,
                                             void* vertex_map_u32_dev, void* face_map_u32_dev, uint32_t capacity_vertices, uint32_t capacity_faces) {
    WDGS_REQUIRE(c, WDGS_E_INVALID, "wdgs_mesh_face_filter_compact: null argument");
    WDGS_REQUIRE(c->selected, WDGS_E_STATE, "filterFaces: no selection precedes the compaction");
    WDGS_REQUIRE(capacity_vertices >= c->kept_v && capacity_faces >= c->kept_f, WDGS_E_CAPACITY, "filterFaces: %u vertices and %u faces, room for %u and %u", c->kept_v,
                 c->kept_f, capacity_vertices, capacity_faces);
    WDGS_REQUIRE((vertices_f32_dev == nullptr) == (vertices_out_f32_dev == nullptr) || c->kept_v == 0, WDGS_E_INVALID,
                 "wdgs_mesh_face_filter_compact: positions need both an input and an output");
    WDGS_REQUIRE(c->kept_f == 0 || faces_out_u32_dev, WDGS_E_INVALID, "wdgs_mesh_face_filter_compact: null faces output");
    WDGS_REQUIRE((((uintptr_t)vertices_f32_dev | (uintptr_t)vertices_out_f32_dev | (uintptr_t)faces_out_u32_dev | (uintptr_t)vertex_map_u32_dev | (uintptr_t)face_map_u32_dev) & 3u) == 0u,
                 WDGS_E_INVALID, "wdgs_mesh_face_filter_compact: misaligned buffer");
    const bool positions = vertices_f32_dev && vertices_out_f32_dev;
    return launch_mesh_emit(c->dev, static_cast<const u32*>(c->faces), c->kept_f ? c->F : 0u, c->kept_v ? c->V : 0u, c->vertex_flags, c->vertex_offsets, c->face_flags,
                            c->face_offsets, positions ? static_cast<const float*>(vertices_f32_dev) : nullptr, positions ? static_cast<float*>(vertices_out_f32_dev) : nullptr,
                            static_cast<u32*>(vertex_map_u32_dev), static_cast<u32*>(faces_out_u32_dev), static_cast<u32*>(face_map_u32_dev));
}
