// Depth compositing: the weights the colour image was composited with, applied to the Gaussians' view-space depths.
// The reference renders colour only and has no counterpart.
//
// depth_composite_kernel walks what rasterize (raster.hip) walks, in the same shape: the walk of tilewalk.h, whose word per entry is the Gaussian's
// 4-byte depth word, kept as z beside the record (36 bytes per record in LDS; no colour).  Records are read by broadcast one iteration ahead of their use,
// two iterations per loop trip.
//
// Per (pixel, record) the alpha is raster.hip's (tilewalk.h), so the weight sum A is the rasterizer's: 1 - A is its alpha texture bit for bit.  On top of
// it one FMA (S = fma(z, w, S)) and the median's two compares and a select; the three colour FMAs and the n_contrib select of rasterize are gone.
// Outputs: A, S / A (one correctly rounded division; 0 where A is not > 0), and the z of the first record at which A reaches 0.5 (0 if none does).  Only
// the images asked for (non-null) are stored.
#include "launch.h"
#include "tilewalk.h"

namespace {

// the inverse of project.hip's ordered_uint
WD_DEV float depth_from_ordered(u32 u) { return wd_bits2f((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u); }

// EXACT: tilewalk.h.  A pixel whose A has become a NaN never reaches the median's threshold either (a comparison): its weight sum is the NaN, its
// expected depth 0 (A > 0 is false), its median what it had before.
template <bool EXACT>
__device__ __attribute__((always_inline)) void depth_body(const RenderSettings& settings, const TileInfo& ti, const u32* __restrict__ splats, u32 num_splats,
                                                          const u32* __restrict__ depths, const u32* __restrict__ sorted_keys,
                                                          const u32* __restrict__ sorted_vals, u32 max_entries, float* __restrict__ out_weight,
                                                          float* __restrict__ out_expected, float* __restrict__ out_median, u32 tile_id, u32 sub, u32 lane,
                                                          u32 total, u32 start, float4* s_geo, float4* s_con, float* s_z) {
    float A = 0.0f, S = 0.0f, M = 0.0f;
    const WalkPixel pix = walk_tile_block<EXACT>(
        settings, ti, splats, num_splats, sorted_keys, sorted_vals, max_entries, tile_id, sub, lane, total, start, s_geo, s_con, A,
        [&](u32 g) { return depths[g]; }, [&](u32 slot, u32 zb) { s_z[slot] = depth_from_ordered(zb); },
        [&](u32 cnt, const WalkPixel& pix) {
            auto composite = [&](const float4 geo, const float4 con, const float z) {
                const float dx = pix.px - geo.x, dy = pix.py - geo.y;
                if (walk_active(pix, geo, dx, dy, A)) {
                    const float w = walk_alpha<EXACT>(con, dx, dy) * (1.0f - A);
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
        });

    if (pix.in_bounds) {
        const size_t p = (size_t)pix.y * pix.W + pix.x;
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

int launch_depth_composite(wdgs_device* dev, const CompositedFrame& f, const u32* depths, float* out_weight, float* out_expected, float* out_median) {
    if (f.ti.total_tiles == 0) return WDGS_OK;
    WDGS_LAUNCH(dev, "depth_composite", depth_composite_kernel, dim3(f.ti.total_tiles), dim3(256), 0, f.st, f.ti, f.splats, f.num_splats, depths, f.ranges,
                f.sorted_keys, f.sorted_vals, f.count_ptr, f.max_batches * 256u /* compat cap, as launch_rasterize */, out_weight, out_expected, out_median, f.nf_stamp, f.nf_frame);
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
