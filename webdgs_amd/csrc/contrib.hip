// Per-Gaussian render contribution: the compositing weights of the frame the last encode rasterized, attributed to the Gaussians
// they belong to.  No reference counterpart: the reference prunes by opacity alone.
//
// Definition.  The *active* (pixel, record) pairs are section 10's: the pixel is inside the image, |dx| <= ex, |dy| <= ey, the pixel's running weight sum A
// is not > 0.99; compat cap and EXACT tiles as in depth.hip.  The pair's weight is w = alpha (1 - A), alpha being raster.hip's and depth.hip's, operation for
// operation (-ffp-contract=off, FMA only where written): w has the compositing weight's bits.  Per Gaussian g, over every active pair whose record is g:
//   sum_q    (u64)  += (u32)(w * 2^24), the conversion truncating -- an integer, so no order of accumulation can change it; the weight sum is sum_q * 2^-24;
//   max_bits (u32)   = max with w's f32 bit pattern (w >= 0: unsigned order is numeric order);
//   pixels   (u32)  += 1 (wraps modulo 2^32).
// A w that is a NaN (EXACT tiles only) adds to none of the three.  One 16-byte record { u64 sum_q; u32 max_bits; u32 pixels; } per Gaussian in a caller-owned
// buffer the call ADDS into: several views accumulate into one buffer, and the result does not depend on the order of views, waves or launches.
//
// contribution_kernel has depth_composite_kernel's walk: one WAVE per 8x8 block, four per 16x16 tile; (key, index) two chunks ahead and the Splat's geometry
// words one chunk ahead; the chunk compacted (ballot + prefix popcount) into a wave-private LDS record set -- centre and extents, the pre-scaled conic with the
// opacity, and the Gaussian's index where depth keeps z; no barrier, a wave stops when its 64 pixels are saturated; tiles dealt round-robin; every tile takes
// this walk, the long ones too (the long-list queue of longlist.h is not touched).  No image is written.
//
// New per (wave, record): the 64 pixels' q summed (u32: 64 * 0.99 * 2^24 < 2^30) and their w bits maximised by two DPP reductions of six steps each
// (row_shr 1, 2, 4, 8, row_bcast 15, row_bcast 31: the total is in lane 63), the pixel count one ballot popcount; all three are put into lane i's registers
// (v_readlane and a select on lane == i), i the record's slot in the chunk, and a record no pixel of the block is active at skips the reductions (uniform branch).  After
// the chunk lane i issues the three global integer atomics of record i, only if its block count is not 0.  No float atomic anywhere.
#include "launch.h"
#include "dmath.h"

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

// EXACT: as in raster.hip and depth.hip -- the tile holds a Splat with a NaN or an infinity among its fp16 fields; every min / clamp / exp in the oracle's form.
template <bool EXACT>
__device__ __attribute__((always_inline)) void contrib_body(const RenderSettings& settings, const TileInfo& ti, const u32* __restrict__ splats, u32 num_splats,
                                                            const u32* __restrict__ sorted_keys, const u32* __restrict__ sorted_vals, u32 max_entries,
                                                            ContribRecord* __restrict__ stats, u32 tile_id, u32 sub, u32 lane, u32 total, u32 start, float4* s_geo,
                                                            float4* s_con, u32* s_idx) {
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

    float A = 0.0f;

    if (!(__any(in_bounds) && start < total)) return;  // 0xFFFFFFFF (empty tile) fails the second test too
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
    // the Splat without its colour: words 0-3 and word 5 (blue | opacity)
    uint2 w01 = make_uint2(0u, 0u), w23 = w01;
    u32 w5 = 0u, gi = 0u;
    if (valid) {
        const u32* sp = splats + (size_t)val_c * 6;
        w01 = *reinterpret_cast<const uint2*>(sp); w23 = *reinterpret_cast<const uint2*>(sp + 2); w5 = sp[5];
        gi = val_c;
    }
    bool dead = false;   // (EXACT; uniform) no pixel of the block can still change its sum
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
            // every pixel of the block is saturated or holds a NaN sum: a record with a NaN alpha at every pixel leaves them as they are and adds nothing
            // (depth.hip and raster.hip drop the same records, so the operations on A stay the same ones)
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
            s_idx[slot] = gi;
        }
        // issue the next chunk's gather and the (key, index) loads of the chunk after it; they land while this chunk composites
        valid = (key_n >> 16u) == want_key && val_n < num_splats;
        if (valid) {
            const u32* sp = splats + (size_t)val_n * 6;
            w01 = *reinterpret_cast<const uint2*>(sp); w23 = *reinterpret_cast<const uint2*>(sp + 2); w5 = sp[5];
            gi = val_n;
        }
        fetch_kv(chunk + 2u, key_n, val_n);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // LDS records written above are read below by other lanes
        __builtin_amdgcn_wave_barrier();

        // lane i's registers: the block's sums of the chunk's record i
        u32 r_sum = 0u, r_max = 0u, r_pix = 0u;
        float4 geo = s_geo[0], con = s_con[0];  // (cnt == 0: a stale record, never used)
#pragma unroll 1
        for (u32 i = 0; i < cnt; i++) {
            const float4 geo_n = s_geo[i + 1u], con_n = s_con[i + 1u];  // (i + 1 <= 64: the spare record) read one iteration ahead
            const float dx = px - geo.x, dy = py - geo.y;
            const bool active = ((int)in_bounds & (int)!(fabsf(dx) > geo.z) & (int)!(fabsf(dy) > geo.w) & (int)!(A > 0.99f)) != 0;
            u32 q = 0u, wb = 0u;
            bool counted = false;
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
        __builtin_amdgcn_wave_barrier();  // all lanes are done reading the records before the next chunk overwrites them
        // every pixel of this wave saturated -> no later record has an active pixel in this block
        if (!__any(in_bounds && !(A > 0.99f))) break;
        if (EXACT) dead = !__any(in_bounds && (A <= 0.99f));   // (false for a saturated and for a NaN sum)
        if (vmask != ~0ull) break;  // the tile's list ended inside this chunk
    }
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

int launch_contribution(wdgs_device* dev, const RenderSettings& st, const TileInfo& ti, const u32* splats, u32 num_splats, const u32* ranges, const u32* sorted_keys,
                        const u32* sorted_vals, const u32* count_ptr, u32 max_batches, void* stats, const u32* nf_stamp, const u32* nf_frame) {
    if (ti.total_tiles == 0) return WDGS_OK;
    const u32 max_entries = max_batches * 256u;  // compat cap, as launch_rasterize
    WDGS_LAUNCH(dev, "contribution", contribution_kernel, dim3(ti.total_tiles), dim3(256), 0, st, ti, splats, num_splats, ranges, sorted_keys, sorted_vals, count_ptr,
                max_entries, (ContribRecord*)stats, nf_stamp, nf_frame);
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}
