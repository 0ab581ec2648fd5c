// SSIM of two rgba8 images (held-out evaluation; no reference counterpart -- the reference has no image metric at all).
//
// Definition: the SSIM of Wang et al. as the 3DGS code base computes it (utils/loss_utils.py::ssim): per rgb channel, values u8/255, an 11x11
// Gaussian window (sigma 1.5, normalised to sum 1) applied as a separable 11-tap filter with ZERO padding, C1 = 0.01^2, C2 = 0.03^2, moments as
// E[x^2] - mu^2; the result is the mean of the per-pixel, per-channel map over 3 W H values.  (Not the clamp-to-edge 5x5 box of loss.hip.)
//
// Numerics: E[x^2] - mu^2 in f32 cancels where the window is flat and bright.  The moments are taken about one shift per output tile and channel,
// s = (a + b) / 2 at the tile's first pixel: every tap reads v - s (a padded tap -s), mu = mu' + s.  The x, y and xy paths run the same operation
// sequence, so identical images give mu_x == mu_y and sigma_x^2 == sigma_y^2 == sigma_xy bit for bit and every map value is exactly 1; the shift is
// symmetric in a and b and every operation commutative, so SSIM(a, b) and SSIM(b, a) agree bit for bit as well.
//
// Shape: a workgroup works 32 x 32 output tiles; the 42 x 42 tile + halo of both images is staged in LDS once (raw rgba8), each channel in turn is
// converted to shifted f32 in LDS, filtered horizontally into LDS (five moments per texel row), then vertically (four output rows per thread).
//
// Reduction: no float atomics and no cross-workgroup hand-off.  The grid is a fixed number of workgroups per device (SSIM_WG_PER_CU per CU) striding
// over the tiles; each writes one f64 partial, and a one-workgroup launch sums the partials in a fixed order.  The partials' scratch (fixed size
// per device) is allocated at the first call and never reallocated, so a recorded command buffer never holds a pointer that goes stale; a device
// that never computes an SSIM allocates nothing.
#include <cmath>

#include "lossimage.h"
#include "ssimwin.h"

namespace {

constexpr u32 ST = SSIM_TILE, RAD = SSIM_RAD;   // output tile edge, window radius
constexpr u32 HT = ST + 2u * RAD;               // staged edge (tile + halo)
constexpr float SSIM_C1 = 0.01f * 0.01f, SSIM_C2 = 0.03f * 0.03f;

__global__ __launch_bounds__(256) void image_ssim_kernel(const u32* __restrict__ a, const u32* __restrict__ b, u32 W, u32 H, u32 tiles_x, u32 n_tiles,
                                                          SsimWindow win, float* __restrict__ map, double* __restrict__ partials) {
    __shared__ float s_lut[256];
    __shared__ u32 s_a[HT][HT], s_b[HT][HT];       // raw rgba8 of tile + halo (0 outside the image: zero padding)
    __shared__ float s_x[HT][HT], s_y[HT][HT];     // one channel, shifted
    __shared__ float s_h[5][HT][ST];               // horizontal pass: E[x], E[y], E[x^2], E[y^2], E[xy] along rows
    __shared__ double s_w[4];
    unorm8_table_fill(s_lut);
    const u32 lx = threadIdx.x & (ST - 1u), ly0 = (threadIdx.x / ST) * 4u;
    double acc = 0.0;
    for (u32 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int bx = (int)((tile % tiles_x) * ST), by = (int)((tile / tiles_x) * ST);
        __syncthreads();   // (the LUT is written; the previous tile's readers are done)
        for (u32 t = threadIdx.x; t < HT * HT; t += 256u) {
            const int hy = (int)(t / HT), hx = (int)(t % HT);
            const int gx = bx + hx - (int)RAD, gy = by + hy - (int)RAD;
            const bool in = gx >= 0 && gx < (int)W && gy >= 0 && gy < (int)H;
            const size_t p = in ? (size_t)gy * W + (size_t)gx : 0;
            s_a[hy][hx] = in ? a[p] : 0u;
            s_b[hy][hx] = in ? b[p] : 0u;
        }
        __syncthreads();
#pragma unroll 1
        for (u32 c = 0; c < 3u; c++) {
            const u32 sh = 8u * c;
            const float s = (unorm8(s_lut, s_a[RAD][RAD], sh) + unorm8(s_lut, s_b[RAD][RAD], sh)) * 0.5f;
            for (u32 t = threadIdx.x; t < HT * HT; t += 256u) {
                const u32 hy = t / HT, hx = t % HT;
                s_x[hy][hx] = unorm8(s_lut, s_a[hy][hx], sh) - s;
                s_y[hy][hx] = unorm8(s_lut, s_b[hy][hx], sh) - s;
            }
            __syncthreads();
            for (u32 t = threadIdx.x; t < HT * ST; t += 256u) {
                const u32 r = t / ST, col = t % ST;
                float m[5];
                window_moments(win, &s_x[r][col], &s_y[r][col], m);
#pragma unroll
                for (u32 q = 0; q < 5u; q++) s_h[q][r][col] = m[q];
            }
            __syncthreads();
            // vertical: four vertically adjacent output pixels per thread share 14 rows of the horizontal moments
            float v[4][5];
            window_slide(win, v, [&](u32 q, u32 j) { return s_h[q][ly0 + j][lx]; });
            const u32 gx = (u32)bx + lx;
#pragma unroll
            for (u32 p = 0; p < 4u; p++) {
                const u32 gy = (u32)by + ly0 + p;
                if (gx >= W || gy >= H) continue;
                const float vx = v[p][2] - v[p][0] * v[p][0];
                const float vy = v[p][3] - v[p][1] * v[p][1];
                const float cxy = v[p][4] - v[p][0] * v[p][1];
                const float mux = v[p][0] + s, muy = v[p][1] + s;
                const float num = (2.0f * (mux * muy) + SSIM_C1) * (2.0f * cxy + SSIM_C2);
                const float den = (mux * mux + muy * muy + SSIM_C1) * (vx + vy + SSIM_C2);
                const float q = wd_div(num, den);
                if (map) map[((size_t)gy * W + gx) * 3u + c] = q;
                acc += (double)q;
            }
        }
    }
#pragma unroll
    for (u32 d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, (int)d, 64);
    if ((threadIdx.x & 63u) == 0u) s_w[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
}

__global__ __launch_bounds__(256) void image_ssim_finish_kernel(const double* __restrict__ partials, u32 n, double count, double* __restrict__ out) {
    __shared__ double s[256];
    double acc = 0.0;
    for (u32 i = threadIdx.x; i < n; i += 256u) acc += partials[i];
    s[threadIdx.x] = acc;
    __syncthreads();
    for (u32 stride = 128u; stride >= 1u; stride >>= 1) {
        if (threadIdx.x < stride) s[threadIdx.x] += s[threadIdx.x + stride];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = s[0] / count;
}

}  // namespace

static SsimWindow make_ssim_window() {
    SsimWindow w;
    double g[SSIM_TAPS], sum = 0.0;
    for (int k = 0; k < (int)SSIM_TAPS; k++) {
        const double d = (double)(k - (int)RAD);
        g[k] = std::exp(-d * d / (2.0 * 1.5 * 1.5));
        sum += g[k];
    }
    for (u32 k = 0; k < SSIM_TAPS; k++) w.g[k] = (float)(g[k] / sum);
    return w;
}
const SsimWindow& ssim_window() {
    static const SsimWindow win = make_ssim_window();
    return win;
}

extern "C" int wdgs_image_ssim_rgb8(wdgs_device* dev, const void* a_rgba8_dev, const void* b_rgba8_dev, uint32_t width, uint32_t height, void* out_f64_dev,
                                    void* map_f32_dev) {
    WDGS_REQUIRE(dev && a_rgba8_dev && b_rgba8_dev && out_f64_dev, WDGS_E_INVALID, "wdgs_image_ssim_rgb8: null argument");
    WDGS_REQUIRE(width > 0 && height > 0, WDGS_E_INVALID, "wdgs_image_ssim_rgb8: empty image (%ux%u)", width, height);
    WDGS_REQUIRE((uint64_t)width * height <= 0x7FFFFFFFull / 3u, WDGS_E_INVALID, "wdgs_image_ssim_rgb8: image too large (%ux%u)", width, height);
    if (!dev->ssim_partials) {
        WDGS_REQUIRE(!dev->capturing, WDGS_E_STATE, "wdgs_image_ssim_rgb8: the first call on a device allocates its scratch and cannot be recorded");
        WDGS_CHECK_HIP(hipSetDevice(dev->ordinal));
        WDGS_CHECK_HIP(hipMalloc(&dev->ssim_partials, sizeof(double) * (size_t)dev->num_cus * SSIM_WG_PER_CU));
        dev->ssim_partials_count = (u32)dev->num_cus * SSIM_WG_PER_CU;
    }
    const SsimWindow& win = ssim_window();
    const u32 tiles_x = ceil_div(width, ST), n_tiles = tiles_x * ceil_div(height, ST);
    WDGS_LAUNCH(dev, "image_ssim", image_ssim_kernel, dim3(dev->ssim_partials_count), dim3(256), 0, (const u32*)a_rgba8_dev, (const u32*)b_rgba8_dev, width, height,
                tiles_x, n_tiles, win, (float*)map_f32_dev, dev->ssim_partials);
    WDGS_CHECK_HIP(hipGetLastError());
    WDGS_LAUNCH(dev, "image_ssim_finish", image_ssim_finish_kernel, dim3(1), dim3(256), 0, (const double*)dev->ssim_partials, dev->ssim_partials_count,
                3.0 * (double)width * (double)height, (double*)out_f64_dev);
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}
