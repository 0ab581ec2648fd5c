// Depth compositing: the weights the colour image was composited with, applied to the Gaussians' view-space depths.
// The reference renders colour only and has no counterpart.
//
// depth_composite_kernel walks what rasterize (raster.hip) walks, in the same shape: one WAVE per 8x8 pixel block, four per 16x16 tile;
//   * the tile's sorted entries in chunks of 64 (lane = entry): (key, index) two chunks ahead, the Splat's geometry words and the Gaussian's
//     4-byte depth word one chunk ahead, in registers;
//   * the chunk compacted (ballot + prefix popcount, order preserving) to the records whose extent box overlaps the wave's block, into a
//     wave-private LDS record set of 36 bytes per record: centre and extents, the pre-scaled conic with the opacity, z.  No colour;
//   * records read by broadcast one iteration ahead of their use, two iterations per loop trip;
//   * no workgroup barrier: a wave stops when its 64 pixels are saturated (A > 0.99) or the tile's entries end;
//   * tiles dealt to the 8 XCDs round-robin (blockIdx order).
// Every tile takes this walk, also the long ones: the long-list task queue of longlist.h is consumed once per forward encode (by rasterize)
// and is not touched here.
//
// Per (pixel, record) the alpha is raster.hip's, operation for operation (-ffp-contract=off, FMA only where written), so the weight sum A is the
// rasterizer's: 1 - A is its alpha texture bit for bit.  On top of it one FMA (S = fma(z, w, S)) and the median's two compares and a select; the
// three colour FMAs and the n_contrib select of rasterize are gone.  Outputs: A, S / A (one correctly rounded division; 0 where A is not > 0), and
// the z of the first record at which A reaches 0.5 (0 if none does).  Only the images asked for (non-null) are stored.
#include "launch.h"
#include "dmath.h"

namespace {

// the inverse of project.hip's ordered_uint
WD_DEV float depth_from_ordered(u32 u) { return wd_bits2f((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u); }

// EXACT: as in raster.hip -- the tile holds a Splat with a NaN or an infinity among its fp16 fields; every min / clamp / exp in the oracle's form, so
// that the finite pixels of such a tile get the rasterizer's weights too.  A pixel whose A has become a NaN never saturates and never reaches the
// median's threshold (both are comparisons): its weight sum is the NaN, its expected depth 0 (A > 0 is false), its median what it had before.
template <bool EXACT>
__device__ __attribute__((always_inline)) void depth_body(const RenderSettings& settings, const TileInfo& ti, const u32* __restrict__ splats, u32 num_splats,
                                                          const u32* __restrict__ depths, const u32* __restrict__ sorted_keys,
                                                          const u32* __restrict__ sorted_vals, u32 max_entries, float* __restrict__ out_weight,
                                                          float* __restrict__ out_expected, float* __restrict__ out_median, u32 tile_id, u32 sub, u32 lane,
                                                          u32 total, u32 start, float4* s_geo, float4* s_con, float* s_z) {
    const u32 tile_x = tile_id % ti.num_tiles_x, tile_y = tile_id / ti.num_tiles_x;
    const u32 bx = tile_x * 16u + (sub & 1u) * 8u, by = tile_y * 16u + (sub >> 1) * 8u;  // block origin
    const u32 pixel_x = bx + (lane & 7u), pixel_y = by + (lane >> 3);
    const float vx = settings.viewport_x, vy = settings.viewport_y;
    const u32 W = wd_to_u32(vx), H = wd_to_u32(vy);
    const bool in_bounds = pixel_x < W && pixel_y < H;
    const float px = (float)pixel_x + 0.5f, py = (float)pixel_y + 0.5f;
    const float blk_x0 = (float)bx + 0.5f, blk_x1 = (float)bx + 7.5f, blk_y0 = (float)by + 0.5f, blk_y1 = (float)by + 7.5f;
    const float cap = (settings.max_splat_radius_px > 0.0f) ? settings.max_splat_radius_px : 1e9f;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;

    float A = 0.0f, S = 0.0f, M = 0.0f;

    if (__any(in_bounds) && start < total) {  // 0xFFFFFFFF (empty tile) fails the second test too
        const u32 want_key = tile_id + 1u;
        auto fetch_kv = [&](u32 c, u32& key, u32& val) {
            const u32 pos = c * 64u + lane;  // position in the tile's list
            const u32 entry = start + pos;
            const bool in_range = entry < total && (max_entries == 0u || pos < max_entries);
            key = in_range ? sorted_keys[entry] : 0u;
            val = in_range ? sorted_vals[entry] : 0xFFFFFFFFu;
        };
        u32 key_c, val_c, key_n, val_n;
        fetch_kv(0u, key_c, val_c);
        fetch_kv(1u, key_n, val_n);
        bool valid = (key_c >> 16u) == want_key && val_c < num_splats;
        // the Splat without its colour: words 0-3 and word 5 (blue | opacity), and the Gaussian's depth word
        uint2 w01 = make_uint2(0u, 0u), w23 = w01;
        u32 w5 = 0u, zb = 0u;
        if (valid) {
            const u32* sp = splats + (size_t)val_c * 6;
            w01 = *reinterpret_cast<const uint2*>(sp); w23 = *reinterpret_cast<const uint2*>(sp + 2); w5 = sp[5];
            zb = depths[val_c];
        }
        bool dead = false;   // (EXACT; uniform) no pixel of the block can still change its sums
        for (u32 chunk = 0;; chunk++) {
            // entries of a tile are contiguous, so the valid lanes are a prefix of the chunk
            const unsigned long long vmask = __ballot(valid);
            if (vmask == 0ull) break;
            // ---- this lane's entry: overlap test against the wave's block (raster.hip: conservative and exact per axis)
            const float cx = (wd_unpack_lo(w01.x) * 0.5f + 0.5f) * vx;
            const float cy = (wd_unpack_hi(w01.x) * -0.5f + 0.5f) * vy;
            const float ex = EXACT ? wd_min(wd_unpack_lo(w01.y), cap) : fminf(wd_unpack_lo(w01.y), cap);
            const float ey = EXACT ? wd_min(wd_unpack_hi(w01.y), cap) : fminf(wd_unpack_hi(w01.y), cap);
            bool ok = valid && !((blk_x0 - cx) > ex || (cx - blk_x1) > ex || (blk_y0 - cy) > ey || (cy - blk_y1) > ey);
            if (EXACT && dead) {
                // every pixel of the block is saturated or holds NaN sums: a record with a NaN alpha at every pixel leaves them as they are (raster.hip drops
                // the same records, so the operations on A stay the same ones)
                const bool nan_rec = __builtin_isunordered(cx, cy) | __builtin_isunordered(wd_unpack_lo(w23.x), wd_unpack_hi(w23.x)) |
                                     __builtin_isunordered(wd_unpack_lo(w23.y), wd_unpack_hi(w5));
                ok = ok && !nan_rec;
            }
            const unsigned long long m = __ballot(ok);
            const u32 cnt = (u32)__popcll(m);
            if (ok) {
                const u32 slot = (u32)__popcll(m & lt_mask);
                s_geo[slot] = make_float4(cx, cy, ex, ey);
                // -0.5 and 2 folded into the conic once per record (powers of two: same bits, raster.hip)
                s_con[slot] = make_float4(-0.5f * wd_unpack_lo(w23.x), -wd_unpack_hi(w23.x), -0.5f * wd_unpack_lo(w23.y), wd_unpack_hi(w5));
                s_z[slot] = depth_from_ordered(zb);
            }
            // issue the next chunk's gather and the (key, index) loads of the chunk after it; they land while this chunk composites
            valid = (key_n >> 16u) == want_key && val_n < num_splats;
            if (valid) {
                const u32* sp = splats + (size_t)val_n * 6;
                w01 = *reinterpret_cast<const uint2*>(sp); w23 = *reinterpret_cast<const uint2*>(sp + 2); w5 = sp[5];
                zb = depths[val_n];
            }
            fetch_kv(chunk + 2u, key_n, val_n);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // LDS records written above are read below by other lanes
            __builtin_amdgcn_wave_barrier();

            auto composite = [&](const float4 geo, const float4 con, const float z) {
                const float dx = px - geo.x, dy = py - geo.y;
                const bool active = ((int)in_bounds & (int)!(fabsf(dx) > geo.z) & (int)!(fabsf(dy) > geo.w) & (int)!(A > 0.99f)) != 0;
                if (active) {
                    const float t1 = __builtin_fmaf(con.x, dx, con.y * dy);
                    const float xe = __builtin_fmaf(t1, dx, (con.z * dy) * dy);  // = -0.5 * power (the record holds the scaled conic)
                    float alpha;
                    if (EXACT) {
                        alpha = wd_clamp(wd_exp(xe) * con.w, 0.0f, 0.99f);
                    } else {
                        const float xc = __builtin_amdgcn_fmed3f(xe, -86.0f, 87.0f);   // (raster.hip: why one clamp of the argument is exact where it matters)
                        alpha = fminf(wd_exp_inrange(xc) * con.w, 0.99f);
                    }
                    const float w = alpha * (1.0f - A);
                    S = __builtin_fmaf(z, w, S);
                    const float An = A + w;
                    // the record at which the weight sum reaches one half (w >= 0: it does so once)
                    M = ((int)(A < 0.5f) & (int)(An >= 0.5f)) ? z : M;
                    A = An;
                }
            };
            if (EXACT) {   // (rare path: the plain loop, fewer live registers)
#pragma unroll 1
                for (u32 i = 0; i < cnt; i++) composite(s_geo[i], s_con[i], s_z[i]);
            } else {
                float4 geo_a = s_geo[0], con_a = s_con[0];  // (cnt == 0: a stale record, never used)
                float z_a = s_z[0];
                for (u32 i = 0; i < cnt; i += 2u) {
                    const float4 geo_b = s_geo[i + 1u], con_b = s_con[i + 1u];  // (i + 1 <= 64: the spare record)
                    const float z_b = s_z[i + 1u];
                    composite(geo_a, con_a, z_a);
                    if (i + 1u >= cnt) break;
                    geo_a = s_geo[i + 2u]; con_a = s_con[i + 2u]; z_a = s_z[i + 2u];   // (i + 2 <= 64)
                    composite(geo_b, con_b, z_b);
                }
            }
            __builtin_amdgcn_wave_barrier();  // all lanes are done reading the records before the next chunk overwrites them
            // every pixel of this wave saturated -> nothing later can change an output of this wave
            if (!__any(in_bounds && !(A > 0.99f))) break;
            if (EXACT) dead = !__any(in_bounds && (A <= 0.99f));   // (false for a saturated and for a NaN sum)
            if (vmask != ~0ull) break;  // the tile's list ended inside this chunk
        }
    }

    if (in_bounds) {
        const size_t p = (size_t)pixel_y * W + pixel_x;
        if (out_weight) out_weight[p] = A;
        if (out_expected) out_expected[p] = (A > 0.0f) ? wd_div(S, A) : 0.0f;
        if (out_median) out_median[p] = M;
    }
}

__global__ __launch_bounds__(256, 8) void depth_composite_kernel(RenderSettings settings, TileInfo ti, const u32* __restrict__ splats, u32 num_splats,
                                                                 const u32* __restrict__ depths, const u32* __restrict__ ranges,
                                                                 const u32* __restrict__ sorted_keys, const u32* __restrict__ sorted_vals,
                                                                 const u32* __restrict__ count_ptr, u32 max_entries, float* __restrict__ out_weight,
                                                                 float* __restrict__ out_expected, float* __restrict__ out_median,
                                                                 const u32* __restrict__ nf_stamp, const u32* __restrict__ nf_frame) {
    // (one record more than a chunk holds: the loop reads one record ahead)
    __shared__ float4 s_geo_all[4][65];  // centre.x, centre.y, extent.x, extent.y   (pixels)
    __shared__ float4 s_con_all[4][65];  // -0.5*conic.x, -conic.y, -0.5*conic.z, opacity
    __shared__ float s_z_all[4][65];     // view-space depth
    const u32 tile_id = blockIdx.x, sub = threadIdx.x >> 6;   // independent waves (no barrier is ever taken): the workgroup is the tile
    const u32 total = *count_ptr;
    const u32 start = ranges[tile_id];
    const bool exact = nf_stamp == nullptr || nf_stamp[tile_id] == *nf_frame;   // (uniform per workgroup)
    if (exact)
        depth_body<true>(settings, ti, splats, num_splats, depths, sorted_keys, sorted_vals, max_entries, out_weight, out_expected, out_median, tile_id, sub,
                         threadIdx.x & 63u, total, start, s_geo_all[sub], s_con_all[sub], s_z_all[sub]);
    else
        depth_body<false>(settings, ti, splats, num_splats, depths, sorted_keys, sorted_vals, max_entries, out_weight, out_expected, out_median, tile_id, sub,
                          threadIdx.x & 63u, total, start, s_geo_all[sub], s_con_all[sub], s_z_all[sub]);
}

// Presentation: inverse depth between the near and the far plane as a grey level, t = clamp((1/z - 1/far) / (1/near - 1/far), 0, 1), grey =
// round(255 t); depth 0 (no weight at the pixel) is black.  Evaluated in f64 (a few thousand pixels per wave, once per saved image).
__global__ __launch_bounds__(256) void depth_to_rgba8_kernel(const float* __restrict__ depth, u32 n, double inv_near, double inv_far, u32* __restrict__ out) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float z = depth[i];
    u32 grey = 0u;
    if (z != 0.0f) {
        double t = (1.0 / (double)z - inv_far) / (inv_near - inv_far);
        t = (t > 0.0) ? ((t < 1.0) ? t : 1.0) : 0.0;   // (a NaN becomes 0)
        grey = (u32)(255.0 * t + 0.5);
    }
    out[i] = grey | (grey << 8) | (grey << 16) | 0xFF000000u;
}

}  // namespace

int launch_depth_composite(wdgs_device* dev, const RenderSettings& st, const TileInfo& ti, const u32* splats, u32 num_splats, const u32* depths, const u32* ranges,
                           const u32* sorted_keys, const u32* sorted_vals, const u32* count_ptr, u32 max_batches, float* out_weight, float* out_expected,
                           float* out_median, const u32* nf_stamp, const u32* nf_frame) {
    if (ti.total_tiles == 0) return WDGS_OK;
    const u32 max_entries = max_batches * 256u;  // compat cap, as launch_rasterize
    WDGS_LAUNCH(dev, "depth_composite", depth_composite_kernel, dim3(ti.total_tiles), dim3(256), 0, st, ti, splats, num_splats, depths, ranges, sorted_keys,
                sorted_vals, count_ptr, max_entries, out_weight, out_expected, out_median, nf_stamp, nf_frame);
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

extern "C" int wdgs_depth_to_rgba8(wdgs_device* dev, const void* depth_f32_dev, uint32_t width, uint32_t height, float near_z, float far_z, void* rgba8_dev) {
    WDGS_REQUIRE(dev && depth_f32_dev && rgba8_dev, WDGS_E_INVALID, "wdgs_depth_to_rgba8: null argument");
    WDGS_REQUIRE(width > 0 && height > 0 && (uint64_t)width * height <= 0x7FFFFFFFull, WDGS_E_INVALID, "wdgs_depth_to_rgba8: bad image size %ux%u", width, height);
    WDGS_REQUIRE(near_z > 0.0f && far_z > near_z && far_z < __builtin_inff(), WDGS_E_INVALID, "wdgs_depth_to_rgba8: need 0 < near < far < inf (got %g, %g)",
                 (double)near_z, (double)far_z);
    const u32 n = width * height;
    WDGS_LAUNCH(dev, "depth_to_rgba8", depth_to_rgba8_kernel, dim3(ceil_div(n, 256u)), dim3(256), 0, (const float*)depth_f32_dev, n, 1.0 / (double)near_z,
                1.0 / (double)far_z, (u32*)rgba8_dev);
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}
