// Per-Gaussian render contribution: the compositing weights of the frame the last encode rasterized, attributed to the Gaussians
// they belong to.  No reference counterpart: the reference prunes by opacity alone.
//
// Definition.  The *active* (pixel, record) pairs are section 10's: the pixel is inside the image, |dx| <= ex, |dy| <= ey, the pixel's running weight sum A
// is not > 0.99; compat cap and EXACT tiles as in depth.hip (tilewalk.h).  The pair's weight is w = alpha (1 - A), alpha being raster.hip's and depth.hip's, operation for
// operation (tilewalk.h's walk_alpha): w has the compositing weight's bits.  Per Gaussian g, over every active pair whose record is g:
//   sum_q    (u64)  += (u32)(w * 2^24), the conversion truncating -- an integer, so no order of accumulation can change it; the weight sum is sum_q * 2^-24;
//   max_bits (u32)   = max with w's f32 bit pattern (w >= 0: unsigned order is numeric order);
//   pixels   (u32)  += 1 (wraps modulo 2^32).
// A w that is a NaN (EXACT tiles only) adds to none of the three.  One 16-byte record { u64 sum_q; u32 max_bits; u32 pixels; } per Gaussian in a caller-owned
// buffer the call ADDS into: several views accumulate into one buffer, and the result does not depend on the order of views, waves or launches.
//
// contribution_kernel takes the walk of tilewalk.h, as depth_composite_kernel does; its word per entry is the Gaussian's index, kept beside the record where
// depth keeps z.  No image is written.
//
// New per (wave, record): the 64 pixels' q summed (u32: 64 * 0.99 * 2^24 < 2^30) and their w bits maximised by two DPP reductions of six steps each
// (row_shr 1, 2, 4, 8, row_bcast 15, row_bcast 31: the total is in lane 63), the pixel count one ballot popcount; all three are put into lane i's registers
// (v_readlane and a select on lane == i), i the record's slot in the chunk, and a record no pixel of the block is active at skips the reductions (uniform branch).  After
// the chunk lane i issues the three global integer atomics of record i, only if its block count is not 0.  No float atomic anywhere.
#include "launch.h"
#include "tilewalk.h"

namespace {

// One step of a wave reduction: lanes whose source is outside the row or masked off by row_mask read 0, the identity of both + and unsigned max
template <int CTRL, int ROW_MASK>
WD_DEV u32 dpp0(u32 x) { return (u32)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, ROW_MASK, 0xf, true); }
WD_DEV u32 umax2(u32 a, u32 b) { return a > b ? a : b; }
// the sum / the maximum of x over the wave's 64 lanes, valid in lane 63
WD_DEV u32 wave_sum_lane63(u32 x) {
    x += dpp0<0x111, 0xf>(x); x += dpp0<0x112, 0xf>(x); x += dpp0<0x114, 0xf>(x); x += dpp0<0x118, 0xf>(x);   // row_shr 1, 2, 4, 8: lane 15 of a row holds the row
    x += dpp0<0x142, 0xa>(x);   // row_bcast15 into rows 1 and 3
    x += dpp0<0x143, 0xc>(x);   // row_bcast31 into rows 2 and 3
    return x;
}
WD_DEV u32 wave_umax_lane63(u32 x) {
    x = umax2(x, dpp0<0x111, 0xf>(x)); x = umax2(x, dpp0<0x112, 0xf>(x)); x = umax2(x, dpp0<0x114, 0xf>(x)); x = umax2(x, dpp0<0x118, 0xf>(x));
    x = umax2(x, dpp0<0x142, 0xa>(x));
    x = umax2(x, dpp0<0x143, 0xc>(x));
    return x;
}

struct ContribRecord { unsigned long long sum_q; u32 max_bits; u32 pixels; };
static_assert(sizeof(ContribRecord) == 16, "the contribution record is 16 bytes (include/webdgs.h)");

// EXACT: tilewalk.h
template <bool EXACT>
__device__ __attribute__((always_inline)) void contrib_body(const RenderSettings& settings, const TileInfo& ti, const u32* __restrict__ splats, u32 num_splats,
                                                            const u32* __restrict__ sorted_keys, const u32* __restrict__ sorted_vals, u32 max_entries,
                                                            ContribRecord* __restrict__ stats, u32 tile_id, u32 sub, u32 lane, u32 total, u32 start, float4* s_geo,
                                                            float4* s_con, u32* s_idx) {
    float A = 0.0f;
    walk_tile_block<EXACT>(
        settings, ti, splats, num_splats, sorted_keys, sorted_vals, max_entries, tile_id, sub, lane, total, start, s_geo, s_con, A,
        [](u32 g) { return g; }, [&](u32 slot, u32 g) { s_idx[slot] = g; },
        [&](u32 cnt, const WalkPixel& pix) {
            // lane i's registers: the block's sums of the chunk's record i
            u32 r_sum = 0u, r_max = 0u, r_pix = 0u;
            float4 geo = s_geo[0], con = s_con[0];  // (cnt == 0: a stale record, never used)
#pragma unroll 1
            for (u32 i = 0; i < cnt; i++) {
                const float4 geo_n = s_geo[i + 1u], con_n = s_con[i + 1u];  // (i + 1 <= 64: the spare record) read one iteration ahead
                const float dx = pix.px - geo.x, dy = pix.py - geo.y;
                u32 q = 0u, wb = 0u;
                bool counted = false;
                if (walk_active(pix, geo, dx, dy, A)) {
                    const float w = walk_alpha<EXACT>(con, dx, dy) * (1.0f - A);
                    A = A + w;
                    counted = !EXACT || w == w;   // (a NaN weight adds to none of the three)
                    if (counted) { q = (u32)(w * 16777216.0f); wb = wd_f2bits(w); }
                }
                const unsigned long long cm = __ballot(counted);
                if (cm != 0ull) {   // (uniform) at least one pixel of the block is active at this record
                    const u32 s = wave_sum_lane63(q), mx = wave_umax_lane63(wb);
                    const u32 s63 = (u32)__builtin_amdgcn_readlane((int)s, 63), mx63 = (u32)__builtin_amdgcn_readlane((int)mx, 63);
                    const bool mine = lane == i;
                    r_sum = mine ? s63 : r_sum; r_max = mine ? mx63 : r_max; r_pix = mine ? (u32)__popcll(cm) : r_pix;
                }
                geo = geo_n; con = con_n;
            }
            // one lane per record: the three integer atomics, for the records with an active pixel in this block
            if (lane < cnt && r_pix != 0u) {
                ContribRecord* rec = stats + s_idx[lane];
                atomicAdd(&rec->sum_q, (unsigned long long)r_sum);
                atomicMax(&rec->max_bits, r_max);
                atomicAdd(&rec->pixels, r_pix);
            }
        });
}

__global__ __launch_bounds__(256, 8) void contribution_kernel(RenderSettings settings, TileInfo ti, const u32* __restrict__ splats, u32 num_splats,
                                                              const u32* __restrict__ ranges, const u32* __restrict__ sorted_keys,
                                                              const u32* __restrict__ sorted_vals, const u32* __restrict__ count_ptr, u32 max_entries,
                                                              ContribRecord* __restrict__ stats, const u32* __restrict__ nf_stamp,
                                                              const u32* __restrict__ nf_frame) {
    // (one record more than a chunk holds: the loop reads one record ahead)
    __shared__ float4 s_geo_all[4][65];  // centre.x, centre.y, extent.x, extent.y   (pixels)
    __shared__ float4 s_con_all[4][65];  // -0.5*conic.x, -conic.y, -0.5*conic.z, opacity
    __shared__ u32 s_idx_all[4][64];     // the Gaussian's index
    const u32 tile_id = blockIdx.x, sub = threadIdx.x >> 6;   // independent waves (no barrier is ever taken): the workgroup is the tile
    const u32 total = *count_ptr;
    const u32 start = ranges[tile_id];
    const bool exact = nf_stamp == nullptr || nf_stamp[tile_id] == *nf_frame;   // (uniform per workgroup)
    if (exact)
        contrib_body<true>(settings, ti, splats, num_splats, sorted_keys, sorted_vals, max_entries, stats, tile_id, sub, threadIdx.x & 63u, total, start,
                           s_geo_all[sub], s_con_all[sub], s_idx_all[sub]);
    else
        contrib_body<false>(settings, ti, splats, num_splats, sorted_keys, sorted_vals, max_entries, stats, tile_id, sub, threadIdx.x & 63u, total, start,
                            s_geo_all[sub], s_con_all[sub], s_idx_all[sub]);
}

}  // namespace

int launch_contribution(wdgs_device* dev, const CompositedFrame& f, void* stats) {
    if (f.ti.total_tiles == 0) return WDGS_OK;
    WDGS_LAUNCH(dev, "contribution", contribution_kernel, dim3(f.ti.total_tiles), dim3(256), 0, f.st, f.ti, f.splats, f.num_splats, f.ranges, f.sorted_keys,
                f.sorted_vals, f.count_ptr, f.max_batches * 256u /* compat cap, as launch_rasterize */, (ContribRecord*)stats, f.nf_stamp, f.nf_frame);
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}
