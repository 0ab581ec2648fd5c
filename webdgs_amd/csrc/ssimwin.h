// The SSIM window and its filter, once, for the held-out metric (ssim.hip) and the exact D-SSIM loss gradient (dssim.hip,
// section 9), whose loss is defined through the metric's map.  Staging, the choice of shift, the LDS layouts and the work splits are each kernel's own.
//
// Both guarantees of the two kernels -- identical images give exactly 1 / exactly 0, and SSIM(a, b) == SSIM(b, a) bit for bit -- rest on what is
// written here: every tap in order k = 0..10, one FMA per tap and moment (-ffp-contract=off: FMAs only where written), the products x*x, y*y, x*y
// rounded on their own first, and the x and y paths the same operation sequence.
#pragma once
#include "common.h"
#include "dmath.h"

// 11 taps of a Gaussian of sigma 1.5, normalised to sum 1, each rounded once to f32 (made on the host, ssim.hip; a kernel argument)
constexpr u32 SSIM_TAPS = 11;
struct SsimWindow { float g[SSIM_TAPS]; };
const SsimWindow& ssim_window();
constexpr u32 SSIM_TILE = 32;   // output tile edge of both kernels
constexpr u32 SSIM_RAD = 5;     // window radius
static_assert(2u * SSIM_RAD + 1u == SSIM_TAPS, "ssim window size");

// The five shifted window moments m = {E[x'], E[y'], E[x'^2], E[y'^2], E[x'y']} of one output along a row, from 11 consecutive values of x' and y'
// (LDS or registers).
WD_DEV void window_moments(const SsimWindow& win, const float* x, const float* y, float m[5]) {
#pragma unroll
    for (u32 q = 0; q < 5u; q++) m[q] = 0.f;
#pragma unroll
    for (u32 k = 0; k < SSIM_TAPS; k++) {
        const float xk = x[k], yk = y[k], g = win.g[k];
        m[0] = __builtin_fmaf(g, xk, m[0]);
        m[1] = __builtin_fmaf(g, yk, m[1]);
        m[2] = __builtin_fmaf(g, xk * xk, m[2]);
        m[3] = __builtin_fmaf(g, yk * yk, m[3]);
        m[4] = __builtin_fmaf(g, xk * yk, m[4]);
    }
}

// The window over Q planes at OUT adjacent outputs, which share their taps: v[o][q] = sum over k of g[k] * load(q, o + k), each output's taps in order
// k = 0..10.  load(q, j): plane q's value at position j of the OUT + 10 the outputs cover; each is loaded once.  Everything unrolls: v stays in registers.
template <u32 OUT, u32 Q, class Load>
__device__ __attribute__((always_inline)) void window_slide(const SsimWindow& win, float (&v)[OUT][Q], Load load) {
#pragma unroll
    for (u32 o = 0; o < OUT; o++)
#pragma unroll
        for (u32 q = 0; q < Q; q++) v[o][q] = 0.f;
#pragma unroll
    for (u32 j = 0; j < OUT + SSIM_TAPS - 1u; j++) {
        float t[Q];
#pragma unroll
        for (u32 q = 0; q < Q; q++) t[q] = load(q, j);
#pragma unroll
        for (u32 o = 0; o < OUT; o++)
            if (j >= o && j - o < SSIM_TAPS) {
#pragma unroll
                for (u32 q = 0; q < Q; q++) v[o][q] = __builtin_fmaf(win.g[j - o], t[q], v[o][q]);
            }
    }
}
