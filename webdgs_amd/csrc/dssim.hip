// Exact D-SSIM loss gradient (dssim_mode "gaussian"; no reference counterpart -- the reference's loss is loss.hip's heuristic).
//
// Loss per view: L = sum over pixels p and rgb channels c of  l1 |d| + l2 d^2 / 2 + ldssim (1 - S[p,c]),  d = x - y, values u8/255 through the
// per-byte table of lossimage.h, S the SSIM map of wdgs_image_ssim_rgb8 (11x11 Gaussian window w, sigma 1.5, zero padding, C1 and C2
// from the training config).  The loss image holds  xyz = l1 sgn(d) + l2 d - ldssim dSum(S)/dx,  w = 1.
//
// Gradient.  With A1 = 2 mx my + C1, A2 = 2 sxy + C2, B1 = mx^2 + my^2 + C1, B2 = sx^2 + sy^2 + C2, S = A1 A2 / (B1 B2), three per-pixel maps
//   delta = 2 (A1/B1 - S) / B2,   gamma = 2 A1 / (B1 B2),   a = 2 S (my/A1 - mx/B1) - mx delta - gamma (my - mx)
// (0 outside the image) give  dSum(S)/dx_p = (w*a)_p + x_p (w*delta)_p + (y_p - x_p) (w*gamma)_p.  my/A1 - mx/B1 is evaluated as
// (my - mx)(my (mx + my) + C1) / (A1 B1), its exact factorisation, so that it vanishes where the means agree.
//
// Numerics.  As in ssim.hip the moments are taken about one shift s per tile and channel, (x + y) / 2 at the tile's centre pixel: every tap
// reads v - s.  The formula keeps its shape under a shift as long as mx in a and x_p are taken about the same s, and every map a tile needs is
// recomputed by the tile itself, so they are.  A1, B1, S and the first term of a use the true means.  Identical images give bit-equal x and y
// moments, so A1 == B1, A2 == B2, S = A1/B1 = 1 and my - mx = y_p - x_p = 0: every term is exactly 0 (the build's -ffp-contract=off keeps the
// x and y operation sequences identical).  No atomics: each output value is one fixed sequence of operations.
//
// Shape: one workgroup per 32 x 32 output tile.  Each thread keeps its share of the 52 x 52 rgba8 tile + 10-pixel halo of both images in registers
// (11 words each); per channel the workgroup converts it to shifted f32 in LDS, filters the five moments over the tile + 5-pixel halo (42 x 42,
// horizontal then vertical pass, several outputs per thread so that neighbouring outputs share their taps), evaluates the three maps there,
// and filters the maps down to the tile (horizontal, then vertical).  LDS: 65 KB, two workgroups per CU.
#include "launch.h"
#include "lossimage.h"
#include "ssimwin.h"

namespace {

constexpr u32 DT = SSIM_TILE, DR = SSIM_RAD, DK = SSIM_TAPS;   // output tile edge, window radius, 11 taps
constexpr u32 ME = DT + 2u * DR;          // 42: map region edge (tile + 5-pixel halo)
constexpr u32 IE = ME + 2u * DR;          // 52: staged input edge (tile + 10-pixel halo)
constexpr u32 IN_WORDS = IE * IE;         // 2704 texels per image
constexpr u32 IN_PER_THREAD = (IN_WORDS + 255u) / 256u;   // 11
constexpr u32 MP = ME + 1u;               // 43: map row pitch (odd: lanes that walk down a column hit distinct banks)
constexpr u32 NP = DT + 1u;               // 33: row pitch of the horizontally filtered maps (likewise)
// LDS region P: the shifted channel of both images (2 x 52 x 52), later the three maps (3 x 42 x 43)
constexpr u32 P_FLOATS = 3u * ME * MP > 2u * IN_WORDS ? 3u * ME * MP : 2u * IN_WORDS;
// LDS region H: the horizontally filtered moments (5 x 52 x 42), later the horizontally filtered maps (3 x 42 x 33)
constexpr u32 H_FLOATS = 5u * IE * ME;
static_assert(3u * ME * NP <= H_FLOATS, "dssim LDS layout");

// work split of the four filter passes (256 threads)
constexpr u32 H1_OUT = 3;                          // moments pass 1: 3 adjacent outputs of a row per item, 52 rows x 14 segments
constexpr u32 H1_SEGS = ME / H1_OUT;
constexpr u32 V1_OUT = 7;                          // moments pass 2: 7 adjacent outputs of a column per item, 42 columns x 6 segments
constexpr u32 V1_ITEMS = ME * (ME / V1_OUT);
constexpr u32 H2_OUT = 4;                          // maps pass 1: 4 adjacent outputs of a row per item, 42 rows x 8 segments
constexpr u32 V2_OUT = 4;                          // maps pass 2: 4 adjacent outputs of a column per thread, 32 columns x 8 segments
static_assert(ME % H1_OUT == 0 && ME % V1_OUT == 0 && V1_ITEMS <= 256u && DT % H2_OUT == 0 && (DT / V2_OUT) * DT == 256u, "dssim work split");

// The three maps of one pixel from its five shifted window moments v = {E[x'], E[y'], E[x'^2], E[y'^2], E[x'y']} (x' = x - s).
WD_DEV void dssim_maps(const float v[5], float s, float c1, float c2, float& ma, float& mdelta, float& mgamma) {
    const float mx = v[0], my = v[1];
    const float vx = v[2] - mx * mx, vy = v[3] - my * my, cxy = v[4] - mx * my;
    const float ux = mx + s, uy = my + s;   // the true means
    const float a1 = 2.0f * (ux * uy) + c1;
    const float b1 = (ux * ux + uy * uy) + c1;
    const float a2 = 2.0f * cxy + c2;
    const float b2 = (vx + vy) + c2;
    const float q1 = a1 / b1, q2 = a2 / b2;
    const float S = q1 * q2;
    const float ib2 = 1.0f / b2;
    const float e = my - mx;
    mgamma = (2.0f * q1) * ib2;
    mdelta = (2.0f * (q1 - S)) * ib2;
    ma = ((2.0f * S) * e) * (uy * (ux + uy) + c1) / (a1 * b1) - mx * mdelta - mgamma * e;
}

__global__ __launch_bounds__(256) void dssim_grad_kernel(u32 W, u32 H, const u32* __restrict__ pred, const u32* __restrict__ targ, wdgs_training_config cfg,
                                                          SsimWindow win, float4* __restrict__ out, int4* __restrict__ acc, u32 acc_quads,
                                                          const u32* __restrict__ acc_dirty) {
    clear_dirty_accumulators(acc, acc_quads, acc_dirty);   // as loss_grad_kernel: backward_rasterize relies on it
    __shared__ float s_lut[256];
    __shared__ float s_p[P_FLOATS];
    __shared__ float s_h[H_FLOATS];
    float* const s_x = s_p;              // [52][52]
    float* const s_y = s_p + IN_WORDS;   // [52][52]
    unorm8_table_fill(s_lut);

    const int bx = (int)(blockIdx.x * DT), by = (int)(blockIdx.y * DT);
    // this thread's share of the staged texels (0 outside the image: zero padding)
    u32 ra[IN_PER_THREAD], rb[IN_PER_THREAD];
#pragma unroll
    for (u32 i = 0; i < IN_PER_THREAD; i++) {
        const u32 t = threadIdx.x + 256u * i;
        const int gx = bx + (int)(t % IE) - (int)(2u * DR), gy = by + (int)(t / IE) - (int)(2u * DR);
        const bool in = t < IN_WORDS && gx >= 0 && gx < (int)W && gy >= 0 && gy < (int)H;
        const size_t p = in ? (size_t)gy * W + (size_t)gx : 0;
        ra[i] = in ? pred[p] : 0u;
        rb[i] = in ? targ[p] : 0u;
    }
    // this thread's output pixels: column lx, rows ly0 .. ly0 + 3 of the tile
    const u32 lx = threadIdx.x & (DT - 1u), ly0 = (threadIdx.x / DT) * V2_OUT;
    const u32 ox = (u32)bx + lx;
    u32 pa[V2_OUT], pb[V2_OUT];
#pragma unroll
    for (u32 k = 0; k < V2_OUT; k++) {
        const u32 oy = (u32)by + ly0 + k;
        const bool in = ox < W && oy < H;
        const size_t p = in ? (size_t)oy * W + ox : 0;
        pa[k] = in ? pred[p] : 0u;
        pb[k] = in ? targ[p] : 0u;
    }
    // the shift: (x + y) / 2 at the tile's centre pixel (clamped into the image).  The second moments' rounding error grows with |mean - s|^2,
    // and a smooth image can change by half its range across the 52 x 52 block: the centre halves the largest distance the first pixel leaves.
    const u32 cx = min((u32)bx + DT / 2u, W - 1u), cy = min((u32)by + DT / 2u, H - 1u);
    const u32 a0 = pred[(size_t)cy * W + cx], b0 = targ[(size_t)cy * W + cx];
    float g[3][V2_OUT];
    __syncthreads();   // (the LUT is written)

#pragma unroll 1
    for (u32 c = 0; c < 3u; c++) {
        const u32 sh = 8u * c;
        const float s = (unorm8(s_lut, a0, sh) + unorm8(s_lut, b0, sh)) * 0.5f;
        // 1. the channel, shifted, into P
#pragma unroll
        for (u32 i = 0; i < IN_PER_THREAD; i++) {
            const u32 t = threadIdx.x + 256u * i;
            if (t < IN_WORDS) {
                s_x[t] = unorm8(s_lut, ra[i], sh) - s;
                s_y[t] = unorm8(s_lut, rb[i], sh) - s;
            }
        }
        __syncthreads();
        // 2. horizontal pass of the moments: H[q][r][col] for rows 0..51, columns 0..41 of the staged block (each output's taps in order k = 0..10)
        for (u32 it = threadIdx.x; it < IE * H1_SEGS; it += 256u) {
            const u32 r = it / H1_SEGS, c0 = (it % H1_SEGS) * H1_OUT;
            float xs[H1_OUT + DK - 1u], ys[H1_OUT + DK - 1u];
#pragma unroll
            for (u32 j = 0; j < H1_OUT + DK - 1u; j++) { xs[j] = s_x[r * IE + c0 + j]; ys[j] = s_y[r * IE + c0 + j]; }
#pragma unroll
            for (u32 o = 0; o < H1_OUT; o++) {
                float m[5];
                window_moments(win, xs + o, ys + o, m);
#pragma unroll
                for (u32 q = 0; q < 5u; q++) s_h[q * IE * ME + r * ME + c0 + o] = m[q];
            }
        }
        __syncthreads();
        // 3. vertical pass of the moments and the maps over the 42 x 42 region (tile + 5-pixel halo) into P as M[m][r][col], pitch MP
        if (threadIdx.x < V1_ITEMS) {
            const u32 col = threadIdx.x % ME, r0 = (threadIdx.x / ME) * V1_OUT;
            float v[V1_OUT][5];
            window_slide(win, v, [&](u32 q, u32 j) { return s_h[q * IE * ME + (r0 + j) * ME + col]; });
            const int gx = bx - (int)DR + (int)col;
#pragma unroll
            for (u32 o = 0; o < V1_OUT; o++) {
                const int gy = by - (int)DR + (int)(r0 + o);
                float ma = 0.f, md = 0.f, mg = 0.f;   // (the maps are 0 outside the image)
                if (gx >= 0 && gx < (int)W && gy >= 0 && gy < (int)H) dssim_maps(v[o], s, cfg.c1, cfg.c2, ma, md, mg);
                const u32 m = (r0 + o) * MP + col;
                s_p[0u * ME * MP + m] = ma; s_p[1u * ME * MP + m] = md; s_p[2u * ME * MP + m] = mg;
            }
        }
        __syncthreads();
        // 4. horizontal pass of the maps: N[m][r][col] for rows 0..41, columns 0..31, pitch NP, into H (lanes walk down the rows)
        for (u32 it = threadIdx.x; it < ME * (DT / H2_OUT); it += 256u) {
            const u32 r = it % ME, c0 = (it / ME) * H2_OUT;
            float n[H2_OUT][3];
            window_slide(win, n, [&](u32 m, u32 j) { return s_p[m * ME * MP + r * MP + c0 + j]; });
#pragma unroll
            for (u32 m = 0; m < 3u; m++)
#pragma unroll
                for (u32 o = 0; o < H2_OUT; o++) s_h[m * ME * NP + r * NP + c0 + o] = n[o][m];
        }
        __syncthreads();
        // 5. vertical pass of the maps down to this thread's four pixels, and the gradient of the channel's SSIM sum
        {
            float n[V2_OUT][3];
            window_slide(win, n, [&](u32 m, u32 j) { return s_h[m * ME * NP + (ly0 + j) * NP + lx]; });
#pragma unroll
            for (u32 o = 0; o < V2_OUT; o++) {
                const float xp = unorm8(s_lut, pa[o], sh) - s, yp = unorm8(s_lut, pb[o], sh) - s;
                g[c][o] = (n[o][0] + xp * n[o][1]) + (yp - xp) * n[o][2];
            }
        }
        // (no barrier here: the next channel writes P, last read in pass 4, and reads H only after its own first barrier)
    }
#pragma unroll
    for (u32 o = 0; o < V2_OUT; o++) {
        const u32 oy = (u32)by + ly0 + o;
        if (ox >= W || oy >= H) continue;
        float4 r;
        r.x = loss_l1_l2(cfg, unorm8(s_lut, pa[o], 0u) - unorm8(s_lut, pb[o], 0u)) - cfg.lambda_dssim * g[0][o];
        r.y = loss_l1_l2(cfg, unorm8(s_lut, pa[o], 8u) - unorm8(s_lut, pb[o], 8u)) - cfg.lambda_dssim * g[1][o];
        r.z = loss_l1_l2(cfg, unorm8(s_lut, pa[o], 16u) - unorm8(s_lut, pb[o], 16u)) - cfg.lambda_dssim * g[2][o];
        r.w = 1.0f;
        out[(size_t)oy * W + ox] = r;
    }
}

}  // namespace

// Same arguments and contract as launch_loss_grad (loss.hip), including the accumulator clear when acc is given.  lambda_dssim == 0 leaves
// only the L1 and L2 terms, which loss_grad computes with the same function (lossimage.h): that launch is taken then, so the two modes agree bit for bit.
int launch_dssim_grad(wdgs_device* dev, u32 W, u32 H, const u32* pred, const u32* targ, const wdgs_training_config& cfg, float4* out, int* acc, u32 acc_rows,
                      const u32* acc_dirty) {
    if (W == 0 || H == 0) return WDGS_OK;
    if (cfg.lambda_dssim == 0.0f) return launch_loss_grad(dev, W, H, pred, targ, cfg, out, acc, acc_rows, acc_dirty);
    WDGS_LAUNCH(dev, "dssim_grad", dssim_grad_kernel, dim3(ceil_div(W, DT), ceil_div(H, DT)), dim3(256), 0, W, H, pred, targ, cfg, ssim_window(), out,
                reinterpret_cast<int4*>(acc), acc_rows * 3u /*12 i32 per row: cleared as int4*/, acc_dirty);
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}
