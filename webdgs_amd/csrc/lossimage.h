// What the kernels that read rgba8 image pairs share: the u8/255 table (loss.hip, dssim.hip, ssim.hip) and, for the two that write a loss image
// (loss_grad_kernel, dssim_grad_kernel), its L1 and L2 terms and the accumulator clear that rides on them.
#pragma once
#include "common.h"
#include "dmath.h"

// rgba8unorm -> f32 through a 256-entry table of i/255, each entry one correctly rounded division, so that a value equals f32(u8)/255 at every use.
// Filled by a workgroup of 256 (a barrier before the first lookup); a lookup takes the texel's byte at bit `shift`.
WD_DEV void unorm8_table_fill(float* lut) { lut[threadIdx.x] = wd_div((float)threadIdx.x, 255.0f); }
WD_DEV float unorm8(const float* lut, u32 texel, u32 shift) { return lut[(texel >> shift) & 0xFFu]; }

WD_DEV float sgn(float v) { return v > 0.0f ? 1.0f : (v < 0.0f ? -1.0f : 0.0f); }

// the L1 and L2 terms of a loss image value, d = prediction - target
WD_DEV float loss_l1_l2(const wdgs_training_config& cfg, float d) { return cfg.lambda_l1 * sgn(d) + cfg.lambda_l2 * d; }

// clearBuffer x4 of the gradient accumulators (tiled-backward-pass.ts:624-627) rides on the loss kernel (a 2-D grid of 256 threads), which precedes
// the backward rasterization anyway: the accumulators' state word (backward_raster.hip) says whether anything has to be cleared at all -- after a
// consuming K17 nothing has -- so the clear is one scalar load here instead of a launch of its own.  acc may be null (compute_loss_only).
WD_DEV void clear_dirty_accumulators(int4* __restrict__ acc, u32 acc_quads, const u32* __restrict__ acc_dirty) {
    if (acc && *acc_dirty != 0u) {
        const int4 z = make_int4(0, 0, 0, 0);
        const u32 nblk = gridDim.x * gridDim.y, blk = blockIdx.y * gridDim.x + blockIdx.x;
        for (u32 i = blk * 256u + threadIdx.x; i < acc_quads; i += nblk * 256u) acc[i] = z;
    }
}
