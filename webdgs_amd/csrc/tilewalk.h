// The tile-list walk depth_composite_kernel (depth.hip) and contribution_kernel (contrib.hip) share (DESIGN.md sections 10 and 11).  It is rasterize's
// (raster.hip) in shape, and off the training path: rasterize keeps its own copy, with what only it has ("What is shared").
//
// One WAVE per 8x8 pixel block, four per 16x16 tile, lane = pixel while compositing and lane = entry while gathering:
//   * the tile's sorted entries in chunks of 64: (key, index) two chunks ahead, the Splat's geometry words (0-3 and 5: no colour) and ONE further 32-bit
//     word per entry, the kernel's own (`gather`: depth's is the depth word, contribution's the Gaussian's index), one chunk ahead, in registers;
//   * the chunk compacted (ballot + prefix popcount, order preserving) to the records whose extent box overlaps the wave's block, into a wave-private LDS
//     record set: s_geo (centre and extents) and s_con (the pre-scaled conic with the opacity), and the kernel's word wherever `keep` puts it;
//   * the kernel composites the chunk's `cnt` records (`chunk_fn`), reading them by broadcast;
//   * no workgroup barrier: a wave stops when its 64 pixels are saturated (A > 0.99) or the tile's entries end;
//   * tiles dealt to the 8 XCDs round-robin (blockIdx order).
// Every tile takes this walk, also the long ones: the long-list task queue of longlist.h is consumed once per forward encode (by rasterize) and is not
// touched here.  max_entries: the compat cap on a tile's list (0 = none), as in rasterize.
//
// EXACT: as in raster.hip -- the tile holds a Splat with a NaN or an infinity among its fp16 fields; every min / clamp / exp in the oracle's form, so
// that the finite pixels of such a tile get the rasterizer's weights too.  A pixel whose A has become a NaN never saturates (a comparison).
//
// Per (pixel, record) the activity test and the alpha are raster.hip's, operation for operation (-ffp-contract=off, FMA only where written):
// walk_active and walk_alpha, so that a kernel's w = alpha (1 - A) has the compositing weight's bits and its A is the rasterizer's.
#pragma once
#include "common.h"
#include "dmath.h"

// The wave's lane as a pixel: its coordinates, its centre, and whether the image holds it
struct WalkPixel {
    u32 x, y, W;
    float px, py;
    bool in_bounds;
};

// the pair is active: the pixel is in the image and inside the record's extent box (geo: centre, extents), and its weight sum is not saturated
WD_DEV bool walk_active(const WalkPixel& pix, const float4 geo, float dx, float dy, float A) {
    return ((int)pix.in_bounds & (int)!(fabsf(dx) > geo.z) & (int)!(fabsf(dy) > geo.w) & (int)!(A > 0.99f)) != 0;
}

// an active pair's alpha (con: the record's scaled conic and opacity; dx, dy: pixel centre - record centre)
template <bool EXACT>
WD_DEV float walk_alpha(const float4 con, float dx, float dy) {
    const float t1 = __builtin_fmaf(con.x, dx, con.y * dy);
    const float xe = __builtin_fmaf(t1, dx, (con.z * dy) * dy);  // = -0.5 * power (the record holds the scaled conic)
    if (EXACT) return wd_clamp(wd_exp(xe) * con.w, 0.0f, 0.99f);
    const float xc = __builtin_amdgcn_fmed3f(xe, -86.0f, 87.0f);   // (raster.hip: why one clamp of the argument is exact where it matters)
    return fminf(wd_exp_inrange(xc) * con.w, 0.99f);
}

// Walks block `sub` of tile `tile_id` (start: the tile's range-table word, total: the frame's entry count).  s_geo, s_con: the wave's record sets, 65 records
// each (one more than a chunk holds, for loops that read one record ahead).  A: the pixel's running weight sum, the kernel's, changed by chunk_fn only.
//   u32  gather(u32 g)             the kernel's word of Gaussian g (g < num_splats), loaded with the Splat
//   void keep(u32 slot, u32 word)  stores it beside record `slot` of the chunk
//   void chunk_fn(u32 cnt, const WalkPixel& pix)   composites records 0 .. cnt - 1, in order (cnt may be 0; all lanes call it)
// Returns the lane's pixel, also where nothing was walked (an empty tile, a block outside the image).
template <bool EXACT, class Gather, class Keep, class ChunkFn>
__device__ __attribute__((always_inline)) WalkPixel walk_tile_block(const RenderSettings& settings, const TileInfo& ti, const u32* __restrict__ splats, u32 num_splats,
                                                                    const u32* __restrict__ sorted_keys, const u32* __restrict__ sorted_vals, u32 max_entries,
                                                                    u32 tile_id, u32 sub, u32 lane, u32 total, u32 start, float4* s_geo, float4* s_con, const float& A,
                                                                    Gather gather, Keep keep, ChunkFn chunk_fn) {
    const u32 tile_x = tile_id % ti.num_tiles_x, tile_y = tile_id / ti.num_tiles_x;
    const u32 bx = tile_x * 16u + (sub & 1u) * 8u, by = tile_y * 16u + (sub >> 1) * 8u;  // block origin
    const float vx = settings.viewport_x, vy = settings.viewport_y;
    WalkPixel pix;
    pix.x = bx + (lane & 7u); pix.y = by + (lane >> 3);
    const u32 W = wd_to_u32(vx), H = wd_to_u32(vy);   // (both in front of the test: converting H only where x is inside is a divergent branch)
    pix.W = W;
    pix.in_bounds = pix.x < W && pix.y < H;
    pix.px = (float)pix.x + 0.5f; pix.py = (float)pix.y + 0.5f;
    const bool in_bounds = pix.in_bounds;
    const float blk_x0 = (float)bx + 0.5f, blk_x1 = (float)bx + 7.5f, blk_y0 = (float)by + 0.5f, blk_y1 = (float)by + 7.5f;
    const float cap = (settings.max_splat_radius_px > 0.0f) ? settings.max_splat_radius_px : 1e9f;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;

    if (!(__any(in_bounds) && start < total)) return pix;  // 0xFFFFFFFF (empty tile) fails the second test too
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
    // the Splat without its colour: words 0-3 and word 5 (blue | opacity), and the kernel's word
    uint2 w01 = make_uint2(0u, 0u), w23 = w01;
    u32 w5 = 0u, wk = 0u;
    if (valid) {
        const u32* sp = splats + (size_t)val_c * 6;
        w01 = *reinterpret_cast<const uint2*>(sp); w23 = *reinterpret_cast<const uint2*>(sp + 2); w5 = sp[5];
        wk = gather(val_c);
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
            // every pixel of the block is saturated or holds NaN sums: a record with a NaN alpha at every pixel leaves them as they are and adds nothing
            // (raster.hip drops the same records, so the operations on A stay the same ones)
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
            keep(slot, wk);
        }
        // issue the next chunk's gather and the (key, index) loads of the chunk after it; they land while this chunk composites
        valid = (key_n >> 16u) == want_key && val_n < num_splats;
        if (valid) {
            const u32* sp = splats + (size_t)val_n * 6;
            w01 = *reinterpret_cast<const uint2*>(sp); w23 = *reinterpret_cast<const uint2*>(sp + 2); w5 = sp[5];
            wk = gather(val_n);
        }
        fetch_kv(chunk + 2u, key_n, val_n);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // LDS records written above are read below by other lanes
        __builtin_amdgcn_wave_barrier();

        chunk_fn(cnt, pix);

        __builtin_amdgcn_wave_barrier();  // all lanes are done reading the records before the next chunk overwrites them
        // every pixel of this wave saturated -> no later record has an active pixel in this block, nothing later can change an output of this wave
        if (!__any(in_bounds && !(A > 0.99f))) break;
        if (EXACT) dead = !__any(in_bounds && (A <= 0.99f));   // (false for a saturated and for a NaN sum)
        if (vmask != ~0ull) break;  // the tile's list ended inside this chunk
    }
    return pix;
}
