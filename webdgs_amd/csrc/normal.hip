// Normal maps: a view-space normal per Gaussian, composited with the weights the colour image was composited with; the normals of a
// depth image; how well the two agree; and a presentation kernel.  The reference renders colour only and has no counterpart.
//
// gaussian_normals_kernel: one thread per Gaussian.  The normal is the Gaussian's shortest axis -- row k of R(q / |q|), k the index of the smallest fp16
// log-scale (ties: the lowest index) -- taken to view space by the upper 3x3 of the camera's view matrix, renormalised, turned toward the camera
// (negated where n . p > 0, p the view-space centre), and packed into one word: octahedral, snorm16 x 2, the z > 0 hemisphere folded (a normal that
// faces the camera has z < 0 and stays in the inner diamond).  NO_NORMAL (0x80008000, which the encoder never produces: it clamps to +-32767) stands
// for a Gaussian without one: |q| = 0, a non-finite half among position, quaternion and log-scales, or a view-space normal that is not finite.
//
// normal_composite_kernel walks what rasterize (raster.hip) walks: the walk of tilewalk.h, whose word per entry is the packed normal, decoded once per
// record into three floats beside it (48 bytes per record in LDS).  Per (pixel, record) the alpha is raster.hip's, so A is depth's weight_sum and
// 1 - A the alpha texture, bit for bit; on top of it three FMAs, N = fma(n, w, N).  depth_body's loop shape: records read one iteration ahead, two
// iterations per trip, the plain loop for EXACT.  No atomics.  Output: float4 {N_x, N_y, N_z, A}, N un-normalised (|N| <= A).
//
// depth_to_normals_kernel: central differences of the back-projected depth image.  normal_agreement_kernel: integer sums (order-free, as metrics.hip's).
#include "launch.h"
#include "tilewalk.h"
#include "wgslm.h"

namespace {

constexpr u32 NO_NORMAL = 0x80008000u;

// ---- the packed word
// octahedral snorm16 x 2 of a unit vector with finite components
WD_DEV u32 normal_encode(vec3 n) {
    const float s = (fabsf(n.x) + fabsf(n.y)) + fabsf(n.z);
    float ox = wd_div(n.x, s), oy = wd_div(n.y, s);
    if (n.z > 0.0f) {   // fold: the outer triangles of the square
        const float fx = __builtin_copysignf(1.0f - fabsf(oy), ox), fy = __builtin_copysignf(1.0f - fabsf(ox), oy);
        ox = fx; oy = fy;
    }
    const float qx = wd_clamp(__builtin_rintf(ox * 32767.0f), -32767.0f, 32767.0f), qy = wd_clamp(__builtin_rintf(oy * 32767.0f), -32767.0f, 32767.0f);
    return ((u32)(int)qx & 0xFFFFu) | ((u32)(int)qy << 16);
}
// The decode DESIGN.md section 12 states, operation by operation in f32 (one rounding each; NO_NORMAL: the zero vector)
WD_DEV vec3 normal_decode(u32 word) {
    if (word == NO_NORMAL) return V3(0.0f);
    const float u = wd_div((float)(int)(short)(word & 0xFFFFu), 32767.0f), v = wd_div((float)(int)(short)(word >> 16), 32767.0f);
    const float au = fabsf(u), av = fabsf(v);
    const float t = (1.0f - au) - av;
    float x = u, y = v;
    if (t < 0.0f) { x = __builtin_copysignf(1.0f - av, u); y = __builtin_copysignf(1.0f - au, v); }
    const float z = -t;
    const float len = wd_sqrt((x * x + y * y) + z * z);
    return V3(wd_div(x, len), wd_div(y, len), wd_div(z, len));
}

WD_DEV bool finite3(vec3 v) { return fabsf(v.x) < __builtin_inff() && fabsf(v.y) < __builtin_inff() && fabsf(v.z) < __builtin_inff(); }

__global__ __launch_bounds__(256) void gaussian_normals_kernel(u32 n, const u32* __restrict__ gaussians, const float* __restrict__ camera_f, u32* __restrict__ normals) {
    const u32 idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= n) return;
    // the record as project.hip's project_one unpacks it: position x y z | raw opacity, quaternion (r, x, y, z), three log-scales | unused
    const u32* g = gaussians + (size_t)idx * 6;
    const uint2 w01 = *reinterpret_cast<const uint2*>(g), w23 = *reinterpret_cast<const uint2*>(g + 2), w45 = *reinterpret_cast<const uint2*>(g + 4);
    // a half is non-finite when its five exponent bits are all ones (project.hip: has_nonfinite_half); the opacity and the unused half do not count
    const u32 M = 0x7C007C00u, C = 0x04000400u;
    const bool nonfinite = ((((w01.x & M) + C) | ((w01.y & 0x7C00u) + 0x0400u) | ((w23.x & M) + C) | ((w23.y & M) + C) | ((w45.x & M) + C) | ((w45.y & 0x7C00u) + 0x0400u)) & 0x80008000u) != 0u;
    const vec4 q = V4(wd_unpack_lo(w23.x), wd_unpack_hi(w23.x), wd_unpack_lo(w23.y), wd_unpack_hi(w23.y));
    const float qq = dot(q, q);   // (halves: no overflow, and 0 only for the zero quaternion)
    if (nonfinite || !(qq > 0.0f)) { normals[idx] = NO_NORMAL; return; }
    const float s0 = wd_unpack_lo(w45.x), s1 = wd_unpack_hi(w45.x), s2 = wd_unpack_lo(w45.y);
    int k = 0;
    float sk = s0;
    if (s1 < sk) { k = 1; sk = s1; }
    if (s2 < sk) k = 2;
    const mat3 R = quat_to_R(q / wd_sqrt(qq));
    const vec3 nw = V3(el(R.c[0], k), el(R.c[1], k), el(R.c[2], k));   // row k
    const CameraUniforms& cam = *reinterpret_cast<const CameraUniforms*>(camera_f);
    const mat4 view = cam.view;
    vec3 nv = normalize(M3(xyz(view.c[0]), xyz(view.c[1]), xyz(view.c[2])) * nw);
    if (!finite3(nv)) { normals[idx] = NO_NORMAL; return; }   // (a view matrix that is singular along nw, or not finite)
    const vec3 p = xyz(view * V4(V3(wd_unpack_lo(w01.x), wd_unpack_hi(w01.x), wd_unpack_lo(w01.y)), 1.0f));   // K1's world_to_view
    if (dot(nv, p) > 0.0f) nv = V3(-nv.x, -nv.y, -nv.z);
    normals[idx] = normal_encode(nv);
}

// ---- compositing.  EXACT: tilewalk.h.  A pixel whose A has become a NaN keeps taking records (its sums are NaNs).
template <bool EXACT>
__device__ __attribute__((always_inline)) void normal_body(const RenderSettings& settings, const TileInfo& ti, const u32* __restrict__ splats, u32 num_splats,
                                                           const u32* __restrict__ normals, const u32* __restrict__ sorted_keys,
                                                           const u32* __restrict__ sorted_vals, u32 max_entries, float4* __restrict__ out, u32 tile_id, u32 sub,
                                                           u32 lane, u32 total, u32 start, float4* s_geo, float4* s_con, float4* s_nrm) {
    float A = 0.0f, Nx = 0.0f, Ny = 0.0f, Nz = 0.0f;
    const WalkPixel pix = walk_tile_block<EXACT>(
        settings, ti, splats, num_splats, sorted_keys, sorted_vals, max_entries, tile_id, sub, lane, total, start, s_geo, s_con, A,
        [&](u32 g) { return normals[g]; },
        [&](u32 slot, u32 word) { const vec3 n = normal_decode(word); s_nrm[slot] = make_float4(n.x, n.y, n.z, 0.0f); },
        [&](u32 cnt, const WalkPixel& pix) {
            auto composite = [&](const float4 geo, const float4 con, const float4 n) {
                const float dx = pix.px - geo.x, dy = pix.py - geo.y;
                if (walk_active(pix, geo, dx, dy, A)) {
                    const float w = walk_alpha<EXACT>(con, dx, dy) * (1.0f - A);
                    Nx = __builtin_fmaf(n.x, w, Nx);
                    Ny = __builtin_fmaf(n.y, w, Ny);
                    Nz = __builtin_fmaf(n.z, w, Nz);
                    A = A + w;
                }
            };
            if (EXACT) {   // (rare path: the plain loop, fewer live registers)
#pragma unroll 1
                for (u32 i = 0; i < cnt; i++) composite(s_geo[i], s_con[i], s_nrm[i]);
            } else {
                float4 geo_a = s_geo[0], con_a = s_con[0], n_a = s_nrm[0];  // (cnt == 0: a stale record, never used)
                for (u32 i = 0; i < cnt; i += 2u) {
                    const float4 geo_b = s_geo[i + 1u], con_b = s_con[i + 1u], n_b = s_nrm[i + 1u];  // (i + 1 <= 64: the spare record)
                    composite(geo_a, con_a, n_a);
                    if (i + 1u >= cnt) break;
                    geo_a = s_geo[i + 2u]; con_a = s_con[i + 2u]; n_a = s_nrm[i + 2u];   // (i + 2 <= 64)
                    composite(geo_b, con_b, n_b);
                }
            }
        });
    if (pix.in_bounds) out[(size_t)pix.y * pix.W + pix.x] = make_float4(Nx, Ny, Nz, A);
}

__global__ __launch_bounds__(256, 8) void normal_composite_kernel(RenderSettings settings, TileInfo ti, const u32* __restrict__ splats, u32 num_splats,
                                                                  const u32* __restrict__ normals, const u32* __restrict__ ranges,
                                                                  const u32* __restrict__ sorted_keys, const u32* __restrict__ sorted_vals,
                                                                  const u32* __restrict__ count_ptr, u32 max_entries, float4* __restrict__ out,
                                                                  const u32* __restrict__ nf_stamp, const u32* __restrict__ nf_frame) {
    // (one record more than a chunk holds: the loop reads one record ahead)
    __shared__ float4 s_geo_all[4][65];  // centre.x, centre.y, extent.x, extent.y   (pixels)
    __shared__ float4 s_con_all[4][65];  // -0.5*conic.x, -conic.y, -0.5*conic.z, opacity
    __shared__ float4 s_nrm_all[4][65];  // the view-space normal (w unused)
    const u32 tile_id = blockIdx.x, sub = threadIdx.x >> 6;   // independent waves (no barrier is ever taken): the workgroup is the tile
    const u32 total = *count_ptr;
    const u32 start = ranges[tile_id];
    const bool exact = nf_stamp == nullptr || nf_stamp[tile_id] == *nf_frame;   // (uniform per workgroup)
    if (exact)
        normal_body<true>(settings, ti, splats, num_splats, normals, sorted_keys, sorted_vals, max_entries, out, tile_id, sub, threadIdx.x & 63u, total, start,
                          s_geo_all[sub], s_con_all[sub], s_nrm_all[sub]);
    else
        normal_body<false>(settings, ti, splats, num_splats, normals, sorted_keys, sorted_vals, max_entries, out, tile_id, sub, threadIdx.x & 63u, total, start,
                           s_geo_all[sub], s_con_all[sub], s_nrm_all[sub]);
}

// ---- the normals of a depth image.  V(i, j) = (ndc_x z / P00, ndc_y z / P11, z), ndc_x = 2 (i + .5) / W - 1, ndc_y = 1 - 2 (j + .5) / H
// (loaders.backprojectDepth); n = normalize(cross(V(i+1, j) - V(i-1, j), V(i, j+1) - V(i, j-1))), turned toward the camera; {n, 1}, or all zero
// where one of the five pixels is outside the image or has no depth (not > 0, or not finite), or the cross product is zero or not finite.  f32, one rounding per operation.
WD_DEV vec3 backproject(const float* __restrict__ depth, u32 i, u32 j, u32 W, float fw, float fh, float p00, float p11, bool& ok) {
    const float z = depth[(size_t)j * W + i];
    ok = ok && (z > 0.0f) && (z < __builtin_inff());
    const float ndc_x = wd_div(2.0f * ((float)i + 0.5f), fw) - 1.0f, ndc_y = 1.0f - wd_div(2.0f * ((float)j + 0.5f), fh);
    return V3(wd_div(ndc_x * z, p00), wd_div(ndc_y * z, p11), z);
}
__global__ __launch_bounds__(256) void depth_to_normals_kernel(const float* __restrict__ depth, float p00, float p11, u32 W, u32 H, float4* __restrict__ out) {
    const u32 p = blockIdx.x * 256u + threadIdx.x;
    if (p >= W * H) return;
    const u32 i = p % W, j = p / W;
    float4 res = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (i >= 1u && i + 1u < W && j >= 1u && j + 1u < H) {
        const float fw = (float)W, fh = (float)H;
        bool ok = true;
        const vec3 c = backproject(depth, i, j, W, fw, fh, p00, p11, ok);
        const vec3 xl = backproject(depth, i - 1u, j, W, fw, fh, p00, p11, ok), xr = backproject(depth, i + 1u, j, W, fw, fh, p00, p11, ok);
        const vec3 yu = backproject(depth, i, j - 1u, W, fw, fh, p00, p11, ok), yd = backproject(depth, i, j + 1u, W, fw, fh, p00, p11, ok);
        const vec3 n = cross(xr - xl, yd - yu);
        const float l2 = dot(n, n);
        if (ok && l2 > 0.0f && l2 < __builtin_inff()) {
            vec3 u = n / wd_sqrt(l2);
            if (dot(u, c) > 0.0f) u = V3(-u.x, -u.y, -u.z);
            if (finite3(u)) res = make_float4(u.x, u.y, u.z, 1.0f);
        }
    }
    out[p] = res;
}

// ---- agreement.  A pixel counts when A >= 0.5, |N| > 0 and the depth normal is valid; c = (N / |N|) . n_d in f32; e = rint(A max(1 - c, 0) 2^24),
// a = rint(A 2^24); out: u64 {sum e, sum a, pixels}, added to with integer atomics (any order gives the same bits).
__global__ __launch_bounds__(256) void normal_agreement_kernel(const float4* __restrict__ comp, const float4* __restrict__ dn, u32 npix, unsigned long long* __restrict__ out) {
    __shared__ unsigned long long s_w[3][4];
    unsigned long long acc_e = 0ull, acc_a = 0ull, acc_n = 0ull;
    for (u32 p = blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += gridDim.x * blockDim.x) {
        const float4 N = comp[p], d = dn[p];
        const float l2 = (N.x * N.x + N.y * N.y) + N.z * N.z;
        if (N.w >= 0.5f && N.w < __builtin_inff() && l2 > 0.0f && l2 < __builtin_inff() && d.w != 0.0f) {
            const float l = wd_sqrt(l2);
            const float c = (wd_div(N.x, l) * d.x + wd_div(N.y, l) * d.y) + wd_div(N.z, l) * d.z;
            const float om = 1.0f - c;
            const float one_minus = (om > 0.0f) ? om : 0.0f;   // (c may exceed 1 by its roundings; a NaN c -- a depth normal that is no number -- counts as 0)
            // (the library's own images have A <= 1 and |n_d| = 1; the cap keeps the conversions defined for any image a host hands in)
            acc_e += (unsigned long long)fminf(__builtin_rintf((N.w * one_minus) * 16777216.0f), 4.0e18f);
            acc_a += (unsigned long long)fminf(__builtin_rintf(N.w * 16777216.0f), 4.0e18f);
            acc_n += 1ull;
        }
    }
#pragma unroll
    for (u32 d = 32; d >= 1; d >>= 1) {
        acc_e += (unsigned long long)__shfl_xor((long long)acc_e, (int)d, 64);
        acc_a += (unsigned long long)__shfl_xor((long long)acc_a, (int)d, 64);
        acc_n += (unsigned long long)__shfl_xor((long long)acc_n, (int)d, 64);
    }
    if ((threadIdx.x & 63u) == 0u) { s_w[0][threadIdx.x >> 6] = acc_e; s_w[1][threadIdx.x >> 6] = acc_a; s_w[2][threadIdx.x >> 6] = acc_n; }
    __syncthreads();
    if (threadIdx.x < 3u) {
        const unsigned long long s = s_w[threadIdx.x][0] + s_w[threadIdx.x][1] + s_w[threadIdx.x][2] + s_w[threadIdx.x][3];
        if (s) atomicAdd(out + threadIdx.x, s);
    }
}

// ---- presentation: rgb = round(255 (0.5 + 0.5 (n_x, -n_y, -n_z))), n = N / |N|, so a surface that faces the camera is the usual blue; black where
// |N| is not > 0; alpha 255.  Evaluated in f64 (once per saved image), as depth_to_rgba8.
__global__ __launch_bounds__(256) void normal_to_rgba8_kernel(const float4* __restrict__ img, u32 n, u32* __restrict__ out) {
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 N = img[i];
    const double x = (double)N.x, y = (double)N.y, z = (double)N.z;
    const double len = __builtin_sqrt((x * x + y * y) + z * z);
    u32 rgb = 0u;
    if (len > 0.0 && len < __builtin_inf()) {
        const u32 r = (u32)(255.0 * (0.5 + 0.5 * (x / len)) + 0.5), g = (u32)(255.0 * (0.5 + 0.5 * (-y / len)) + 0.5), b = (u32)(255.0 * (0.5 + 0.5 * (-z / len)) + 0.5);
        rgb = r | (g << 8) | (b << 16);
    }
    out[i] = rgb | 0xFF000000u;
}

}  // namespace

int launch_gaussian_normals(wdgs_device* dev, u32 n, const u32* gaussians, const float* camera, u32* normals) {
    if (n == 0) return WDGS_OK;
    WDGS_LAUNCH(dev, "gaussian_normals", gaussian_normals_kernel, dim3(ceil_div(n, 256u)), dim3(256), 0, n, gaussians, camera, normals);
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

int launch_normal_composite(wdgs_device* dev, const CompositedFrame& f, const u32* normals, float4* out) {
    if (f.ti.total_tiles == 0) return WDGS_OK;
    WDGS_LAUNCH(dev, "normal_composite", normal_composite_kernel, dim3(f.ti.total_tiles), dim3(256), 0, f.st, f.ti, f.splats, f.num_splats, normals, f.ranges,
                f.sorted_keys, f.sorted_vals, f.count_ptr, f.max_batches * 256u /* compat cap, as launch_rasterize */, out, f.nf_stamp, f.nf_frame);
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

static bool image_size_ok(uint32_t width, uint32_t height) { return width > 0 && height > 0 && (uint64_t)width * height <= 0x7FFFFFFFull; }

extern "C" int wdgs_depth_to_normals(wdgs_device* dev, const void* depth_f32_dev, uint32_t width, uint32_t height, float p00, float p11, void* normals_rgba32f_dev) {
    WDGS_REQUIRE(dev && depth_f32_dev && normals_rgba32f_dev, WDGS_E_INVALID, "wdgs_depth_to_normals: null argument");
    WDGS_REQUIRE(image_size_ok(width, height), WDGS_E_INVALID, "wdgs_depth_to_normals: bad image size %ux%u", width, height);
    WDGS_REQUIRE(p00 != 0.0f && p11 != 0.0f && std::fabs(p00) < __builtin_inff() && std::fabs(p11) < __builtin_inff(), WDGS_E_INVALID,
                 "wdgs_depth_to_normals: proj[0][0] and proj[1][1] must be finite and non-zero (got %g, %g)", (double)p00, (double)p11);
    WDGS_REQUIRE(((uintptr_t)normals_rgba32f_dev & 15u) == 0u, WDGS_E_INVALID, "wdgs_depth_to_normals: the output image must be 16-byte aligned");
    WDGS_LAUNCH(dev, "depth_to_normals", depth_to_normals_kernel, dim3(ceil_div(width * height, 256u)), dim3(256), 0, (const float*)depth_f32_dev, p00, p11, width, height,
                (float4*)normals_rgba32f_dev);
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

extern "C" int wdgs_normal_agreement(wdgs_device* dev, const void* normal_rgba32f_dev, const void* depth_normals_rgba32f_dev, uint32_t width, uint32_t height,
                                     void* out_u64x3_dev) {
    WDGS_REQUIRE(dev && normal_rgba32f_dev && depth_normals_rgba32f_dev && out_u64x3_dev, WDGS_E_INVALID, "wdgs_normal_agreement: null argument");
    WDGS_REQUIRE(image_size_ok(width, height), WDGS_E_INVALID, "wdgs_normal_agreement: bad image size %ux%u", width, height);
    WDGS_REQUIRE((((uintptr_t)normal_rgba32f_dev | (uintptr_t)depth_normals_rgba32f_dev) & 15u) == 0u && ((uintptr_t)out_u64x3_dev & 7u) == 0u, WDGS_E_INVALID,
                 "wdgs_normal_agreement: the images must be 16-byte aligned, the sums 8-byte aligned");
    WDGS_CHECK_HIP(hipMemsetAsync(out_u64x3_dev, 0, 24, dev->stream));
    const u32 n = width * height;
    const u32 grid = std::min<u32>(ceil_div(n, 256u), (u32)dev->num_cus * 4u);
    WDGS_LAUNCH(dev, "normal_agreement", normal_agreement_kernel, dim3(grid), dim3(256), 0, (const float4*)normal_rgba32f_dev, (const float4*)depth_normals_rgba32f_dev, n,
                (unsigned long long*)out_u64x3_dev);
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

extern "C" int wdgs_normal_to_rgba8(wdgs_device* dev, const void* normal_rgba32f_dev, uint32_t width, uint32_t height, void* rgba8_dev) {
    WDGS_REQUIRE(dev && normal_rgba32f_dev && rgba8_dev, WDGS_E_INVALID, "wdgs_normal_to_rgba8: null argument");
    WDGS_REQUIRE(image_size_ok(width, height), WDGS_E_INVALID, "wdgs_normal_to_rgba8: bad image size %ux%u", width, height);
    WDGS_REQUIRE(((uintptr_t)normal_rgba32f_dev & 15u) == 0u, WDGS_E_INVALID, "wdgs_normal_to_rgba8: the image must be 16-byte aligned");
    const u32 n = width * height;
    WDGS_LAUNCH(dev, "normal_to_rgba8", normal_to_rgba8_kernel, dim3(ceil_div(n, 256u)), dim3(256), 0, (const float4*)normal_rgba32f_dev, n, (u32*)rgba8_dev);
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}
