// TSDF fusion of depth maps and mesh extraction by marching tetrahedra (no counterpart in the reference, which renders colour only).
//
// The volume is an axis-aligned grid of voxels, x fastest: voxel (i, j, k) has the linear index (k ny + j) nx + i and its centre at
// origin + (i + 1/2, j + 1/2, k + 1/2) voxel_size.  tsdf and weight are f32 per voxel; the optional colour is three f32 PLANES (r, g, b: rgb[c n + index]),
// so that every array a wave touches is read and written as whole 256-byte rows.  Everything here is f32 in the order written (-ffp-contract=off):
// tests/tsdf64.py restates it operation by operation.
#include <algorithm>
#include <cmath>
#include <memory>

#include "launch.h"

namespace {

struct TsdfGrid {
    float ox, oy, oz, voxel_size;
    u32 nx, ny, nz;
};

// Centre of voxel i along one axis: origin + ((float)i + 0.5) voxel_size, two roundings (i + 0.5 is exact below 2^23).  integrate and the mesh use this one form.
__device__ __forceinline__ float voxel_centre(float o, u32 i, float vs) { return o + ((float)i + 0.5f) * vs; }

// ---- integrate: one thread per voxel, no atomics.  A wave owns 64 consecutive x of one (j, k) row, a block four such rows; a lane whose voxel is skipped loads
// and stores nothing of the volume, so a wave whose voxels all fall outside the frustum touches only the camera block (scalar loads).
__global__ __launch_bounds__(256) void tsdf_integrate_kernel(TsdfGrid g, float truncation, float max_weight, const float* __restrict__ camera, const float* __restrict__ depth,
                                                             const float* __restrict__ weight_sum, const u32* __restrict__ colour, u32 W, u32 H, float min_weight_sum,
                                                             u32 x_blocks, u32 rows, float* __restrict__ tsdf, float* __restrict__ weight, float* __restrict__ rgb) {
    const u32 row = blockIdx.x * 4u + (threadIdx.x >> 6);   // wave-uniform
    if (row >= rows) return;
    const u32 xb = row % x_blocks, jk = row / x_blocks;
    const u32 j = jk % g.ny, k = jk / g.ny;
    const u32 i = xb * 64u + (threadIdx.x & 63u);
    if (i >= g.nx) return;
    const float cx = voxel_centre(g.ox, i, g.voxel_size), cy = voxel_centre(g.oy, j, g.voxel_size), cz = voxel_centre(g.oz, k, g.voxel_size);
    // v = view (c, 1): the view matrix is floats 0-15 of the block, column-major; products rounded, summed left to right
    const float vx = ((camera[0] * cx + camera[4] * cy) + camera[8] * cz) + camera[12];
    const float vy = ((camera[1] * cx + camera[5] * cy) + camera[9] * cz) + camera[13];
    const float z = ((camera[2] * cx + camera[6] * cy) + camera[10] * cz) + camera[14];
    if (!(z > 0.0f)) return;
    const float fw = (float)W, fh = (float)H;
    if (!(camera[64] == fw && camera[65] == fh)) return;   // a block of another image size (uniform): nothing is written
    const float px = (((camera[32] * vx) / z) * 0.5f + 0.5f) * fw;
    const float py = ((((-camera[37]) * vy) / z) * 0.5f + 0.5f) * fh;
    if (!(px >= 0.0f && px < fw && py >= 0.0f && py < fh)) return;   // (a NaN fails every comparison)
    const u32 p = (u32)py * W + (u32)px;   // px < fw, so (u32)px <= W - 1: inside the image
    const float d = depth[p];
    if (!(d > 0.0f && d < __builtin_inff())) return;
    if (weight_sum && !(weight_sum[p] >= min_weight_sum)) return;
    const float sdf = d - z;
    if (sdf < -truncation) return;
    const float t = fminf(sdf / truncation, 1.0f);
    const size_t n = (size_t)g.nx * g.ny * g.nz, v = ((size_t)k * g.ny + j) * g.nx + i;
    const float T = tsdf[v], Wt = weight[v];
    const float q = Wt + 1.0f;
    tsdf[v] = (T * Wt + t) / q;
    if (colour && rgb) {
        const u32 c = colour[p];
        rgb[v] = (rgb[v] * Wt + (float)(c & 255u) / 255.0f) / q;
        rgb[n + v] = (rgb[n + v] * Wt + (float)((c >> 8) & 255u) / 255.0f) / q;
        rgb[2u * n + v] = (rgb[2u * n + v] * Wt + (float)((c >> 16) & 255u) / 255.0f) / q;
    }
    weight[v] = fminf(q, max_weight);
}

__global__ __launch_bounds__(256) void tsdf_reset_kernel(size_t n, float* __restrict__ tsdf) {
    for (size_t v = (size_t)blockIdx.x * 256u + threadIdx.x; v < n; v += (size_t)gridDim.x * 256u) tsdf[v] = 1.0f;
}

// ---- marching tetrahedra on the Kuhn split of a cell.  Corner c of a cell is the voxel at the offset (c & 1, c >> 1 & 1, c >> 2 & 1).  Tetrahedron t has the
// corners {0, e_a, e_a + e_b, 7} for the t-th permutation (a, b, c) of the axes in the order xyz, xzy, yxz, yzx, zxy, zyx; det(p1 - p0, p2 - p0, p3 - p0) is the
// permutation's sign, so tetrahedra 0, 3, 4 are positively oriented and 1, 2, 5 negatively.
__device__ constexpr unsigned char TET_CORNER[6][4] = {{0, 1, 3, 7}, {0, 1, 5, 7}, {0, 2, 3, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 4, 6, 7}};
__device__ constexpr unsigned char TET_NEGATIVE[6] = {0, 1, 1, 0, 0, 1};

// The 16 cases, derived, for a POSITIVELY oriented tetrahedron (p0 .. p3); bit v of the case is set when p_v is inside (T < 0).  A triangle vertex is the edge
// {u, v} of the tetrahedron, packed u | v << 2; a negatively oriented tetrahedron swaps the last two vertices of each triangle.
//   one corner a apart from the others b < c < d (a alone inside, or alone outside): the triangle {a,b}, {a,c}, {a,d}.  With (a, b, c, d) an even permutation of
//     (0, 1, 2, 3) the tetrahedron (a, b, c, d) is positively oriented and that order turns counter-clockwise seen from the side away from a: kept when a is the
//     inside corner, its last two swapped when a is the outside one; the reverse for an odd permutation.
//   two inside a < b, two outside c < d: the quadrilateral q0 = {a,c}, q1 = {a,d}, q2 = {b,d}, q3 = {b,c} as (q0, q1, q2), (q0, q2, q3), which turns
//     counter-clockwise seen from the side of c and d when (a, b, c, d) is even; for an odd one (q0, q2, q1), (q0, q3, q2).
struct TetCase { unsigned char count; unsigned char edge[2][3]; };
constexpr bool perm_even(int a, int b, int c, int d) {
    const int p[4] = {a, b, c, d};
    int inv = 0;
    for (int x = 0; x < 4; x++)
        for (int y = x + 1; y < 4; y++) inv += p[x] > p[y];
    return (inv & 1) == 0;
}
constexpr unsigned char tet_edge(int u, int v) { return (unsigned char)(u | (v << 2)); }
constexpr TetCase tet_case(int mask) {
    TetCase r = {0, {{0, 0, 0}, {0, 0, 0}}};
    int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, ni = 0, no = 0;
    for (int v = 0; v < 4; v++) {
        if (mask >> v & 1) in[ni++] = v;
        else out[no++] = v;
    }
    if (ni == 1 || ni == 3) {
        const int a = (ni == 1) ? in[0] : out[0];
        const int* o = (ni == 1) ? out : in;
        const bool keep = perm_even(a, o[0], o[1], o[2]) == (ni == 1);
        r.count = 1;
        r.edge[0][0] = tet_edge(a, o[0]);
        r.edge[0][1] = tet_edge(a, keep ? o[1] : o[2]);
        r.edge[0][2] = tet_edge(a, keep ? o[2] : o[1]);
    } else if (ni == 2) {
        const unsigned char q0 = tet_edge(in[0], out[0]), q1 = tet_edge(in[0], out[1]), q2 = tet_edge(in[1], out[1]), q3 = tet_edge(in[1], out[0]);
        const bool even = perm_even(in[0], in[1], out[0], out[1]);
        r.count = 2;
        r.edge[0][0] = q0; r.edge[0][1] = even ? q1 : q2; r.edge[0][2] = even ? q2 : q1;
        r.edge[1][0] = q0; r.edge[1][1] = even ? q2 : q3; r.edge[1][2] = even ? q3 : q2;
    }
    return r;
}
__device__ constexpr TetCase TET_CASES[16] = {tet_case(0), tet_case(1), tet_case(2),  tet_case(3),  tet_case(4),  tet_case(5),  tet_case(6),  tet_case(7),
                                              tet_case(8), tet_case(9), tet_case(10), tet_case(11), tet_case(12), tet_case(13), tet_case(14), tet_case(15)};

// The eight corners of cell `cell` (linear over (nx-1)(ny-1)(nz-1), x fastest): bit c of the result is set when corner c is inside (T < 0; a T of 0 is outside),
// bit 8 when the cell is valid (every corner's weight >= min_weight).  Consecutive lanes hold consecutive x: every load is a run of consecutive floats.
__device__ __forceinline__ u32 load_cell(const TsdfGrid& g, u32 cell, const float* __restrict__ tsdf, const float* __restrict__ weight, float min_weight, u32& i, u32& j,
                                         u32& k) {
    const u32 cx = g.nx - 1u, cy = g.ny - 1u;
    i = cell % cx;
    const u32 r = cell / cx;
    j = r % cy;
    k = r / cy;
    u32 bits = 0x100u;
#pragma unroll
    for (u32 n = 0; n < 8u; n++) {
        const size_t v = ((size_t)(k + (n >> 2)) * g.ny + (j + ((n >> 1) & 1u))) * g.nx + (i + (n & 1u));
        if (tsdf[v] < 0.0f) bits |= 1u << n;
        if (!(weight[v] >= min_weight)) bits &= ~0x100u;
    }
    return bits;
}

__device__ __forceinline__ u32 tet_mask(u32 inside, u32 t) {
    u32 m = 0u;
#pragma unroll
    for (u32 v = 0; v < 4u; v++) m |= ((inside >> TET_CORNER[t][v]) & 1u) << v;
    return m;
}

__global__ __launch_bounds__(256) void tsdf_count_kernel(TsdfGrid g, u32 cells, const float* __restrict__ tsdf, const float* __restrict__ weight, float min_weight,
                                                         u32* __restrict__ counts) {
    const u32 cell = blockIdx.x * 256u + threadIdx.x;
    if (cell >= cells) return;
    u32 i, j, k;
    const u32 c = load_cell(g, cell, tsdf, weight, min_weight, i, j, k);
    u32 n = 0u;
    if (c & 0x100u) {
#pragma unroll
        for (u32 t = 0; t < 6u; t++) n += TET_CASES[tet_mask(c, t)].count;
    }
    counts[cell] = n;
}

// Writes the triangles of every cell at its scanned offset: cells in linear order, then tetrahedron order, then the case's triangle order.  A vertex on the lattice
// edge between the corners A and B -- A the one with the lower linear voxel index, which on a Kuhn edge is the one whose offset bits are a subset of B's -- is
// pA + (pB - pA) (T_A / (T_A - T_B)) per axis, so every cell and tetrahedron that touches the edge writes the same bits; its key is
// linear_index(A) 8 + (dx + 2 dy + 4 dz - 1), (dx, dy, dz) the offset from A to B.
__global__ __launch_bounds__(256) void tsdf_emit_kernel(TsdfGrid g, u32 cells, const float* __restrict__ tsdf, const float* __restrict__ weight, const float* __restrict__ rgb,
                                                        float min_weight, const u32* __restrict__ counts, const u32* __restrict__ offsets,
                                                        float* __restrict__ positions, unsigned long long* __restrict__ keys, u32* __restrict__ colours) {
    const u32 cell = blockIdx.x * 256u + threadIdx.x;
    if (cell >= cells) return;
    u32 i, j, k;
    const u32 c = load_cell(g, cell, tsdf, weight, min_weight, i, j, k);
    if (!(c & 0x100u)) return;
    const size_t n = (size_t)g.nx * g.ny * g.nz;
    size_t tri = offsets[cell];
    // (a volume written behind the library's back since the count -- through a pointer handed out earlier -- may hold other cases now: a cell never
    // writes more triangles than were counted for it, so the output stays inside the `total` the caller made room for)
    const size_t end = tri + counts[cell];
    for (u32 t = 0; t < 6u; t++) {
        const TetCase& tc = TET_CASES[tet_mask(c, t)];   // (read where it lies: a copy indexed at run time would live in scratch)
        for (u32 f = 0; f < tc.count && tri < end; f++, tri++) {
            for (u32 s = 0; s < 3u; s++) {
                const u32 slot = (TET_NEGATIVE[t] && s != 0u) ? 3u - s : s;   // a negatively oriented tetrahedron turns the other way
                const u32 e = tc.edge[f][slot];
                u32 a = TET_CORNER[t][e & 3u], b = TET_CORNER[t][e >> 2];
                if (a > b) { const u32 x = a; a = b; b = x; }   // the corners of a tetrahedron are nested offsets: the smaller is A
                const u32 d = a ^ b;
                const u32 ai = i + (a & 1u), aj = j + ((a >> 1) & 1u), ak = k + (a >> 2);
                const size_t va = ((size_t)ak * g.ny + aj) * g.nx + ai;
                const size_t vb = ((size_t)(ak + (d >> 2)) * g.ny + (aj + ((d >> 1) & 1u))) * g.nx + (ai + (d & 1u));
                const float TA = tsdf[va], TB = tsdf[vb];
                const float w = TA / (TA - TB);
                const float ax = voxel_centre(g.ox, ai, g.voxel_size), ay = voxel_centre(g.oy, aj, g.voxel_size), az = voxel_centre(g.oz, ak, g.voxel_size);
                float* p = positions + (tri * 3u + s) * 3u;
                p[0] = (d & 1u) ? ax + (voxel_centre(g.ox, ai + 1u, g.voxel_size) - ax) * w : ax;
                p[1] = (d & 2u) ? ay + (voxel_centre(g.oy, aj + 1u, g.voxel_size) - ay) * w : ay;
                p[2] = (d & 4u) ? az + (voxel_centre(g.oz, ak + 1u, g.voxel_size) - az) * w : az;
                if (keys) keys[tri * 3u + s] = (unsigned long long)va * 8ull + (d - 1u);
                if (colours) {
                    u32 word = 0xFF000000u;
#pragma unroll
                    for (u32 ch = 0; ch < 3u; ch++) {
                        const float ca = rgb[ch * n + va], cb = rgb[ch * n + vb];
                        const float cv = fminf(fmaxf(ca + (cb - ca) * w, 0.0f), 1.0f);   // (fmaxf drops a NaN: 0)
                        word |= (u32)(cv * 255.0f + 0.5f) << (8u * ch);
                    }
                    colours[tri * 3u + s] = word;
                }
            }
        }
    }
}

}  // namespace

// ---------------------------------------------------------------- launchers
struct TsdfLaunchGrid {
    TsdfGrid g;
    size_t voxels;
    u32 cells;
};
static TsdfLaunchGrid tsdf_grid(const float origin[3], float voxel_size, const u32 dims[3]) {
    TsdfLaunchGrid l;
    l.g = TsdfGrid{origin[0], origin[1], origin[2], voxel_size, dims[0], dims[1], dims[2]};
    l.voxels = (size_t)dims[0] * dims[1] * dims[2];
    l.cells = (dims[0] - 1u) * (dims[1] - 1u) * (dims[2] - 1u);
    return l;
}

int launch_tsdf_reset(wdgs_device* dev, size_t voxels, float* tsdf, float* weight, float* rgb) {
    const u32 grid = (u32)std::min<size_t>((voxels + 255u) / 256u, 65536u);
    WDGS_LAUNCH(dev, "tsdf_reset", tsdf_reset_kernel, dim3(grid), dim3(256), 0, voxels, tsdf);
    WDGS_CHECK_HIP(hipGetLastError());
    WDGS_CHECK_HIP(hipMemsetAsync(weight, 0, voxels * sizeof(float), dev->stream));
    if (rgb) WDGS_CHECK_HIP(hipMemsetAsync(rgb, 0, 3u * voxels * sizeof(float), dev->stream));
    return WDGS_OK;
}

int launch_tsdf_integrate(wdgs_device* dev, const float origin[3], float voxel_size, const u32 dims[3], float truncation, float max_weight, const float* camera,
                          const float* depth, const float* weight_sum, const u32* colour, u32 width, u32 height, float min_weight_sum, float* tsdf, float* weight,
                          float* rgb) {
    const TsdfLaunchGrid l = tsdf_grid(origin, voxel_size, dims);
    const u32 x_blocks = ceil_div(dims[0], 64u);
    const u32 rows = x_blocks * dims[1] * dims[2];   // <= nx ny nz <= 2^28
    WDGS_LAUNCH(dev, "tsdf_integrate", tsdf_integrate_kernel, dim3(ceil_div(rows, 4u)), dim3(256), 0, l.g, truncation, max_weight, camera, depth, weight_sum, colour, width,
                height, min_weight_sum, x_blocks, rows, tsdf, weight, rgb);
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

int launch_tsdf_count(wdgs_device* dev, const float origin[3], float voxel_size, const u32 dims[3], const float* tsdf, const float* weight, float min_weight, u32* counts) {
    const TsdfLaunchGrid l = tsdf_grid(origin, voxel_size, dims);
    WDGS_LAUNCH(dev, "tsdf_count", tsdf_count_kernel, dim3(ceil_div(l.cells, 256u)), dim3(256), 0, l.g, l.cells, tsdf, weight, min_weight, counts);
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

int launch_tsdf_emit(wdgs_device* dev, const float origin[3], float voxel_size, const u32 dims[3], const float* tsdf, const float* weight, const float* rgb, float min_weight,
                     const u32* counts, const u32* offsets, float* positions, unsigned long long* keys, u32* colours) {
    const TsdfLaunchGrid l = tsdf_grid(origin, voxel_size, dims);
    WDGS_LAUNCH(dev, "tsdf_emit", tsdf_emit_kernel, dim3(ceil_div(l.cells, 256u)), dim3(256), 0, l.g, l.cells, tsdf, weight, rgb, min_weight, counts, offsets, positions,
                keys, colours);
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

// ---------------------------------------------------------------- the C ABI object (include/webdgs.h: wdgs_tsdf_volume)
struct wdgs_tsdf_volume {
    wdgs_device* dev = nullptr;
    float origin[3] = {0.f, 0.f, 0.f};
    float voxel_size = 0.f, truncation = 0.f, max_weight = 0.f;
    u32 dims[3] = {0, 0, 0};
    size_t voxels = 0;
    u32 cells = 0;
    DevMem<float> tsdf, weight, rgb;   // rgb empty for a volume without colour
    DevMem<u32> counts, offsets;       // per cell: the triangle count and its exclusive scan
    DevMem<u32> total;                 // one word: the scan's grand total
    ScanScratch scan;
    // emit_triangles is valid only for the volume count_triangles saw: every call that writes the volume, or hands out a pointer a host may write through, moves on
    uint64_t generation = 1, counted_generation = 0;
    u32 counted_total = 0;
    float counted_min_weight = 0.f;
};

static bool positive_finite(float x) { return x > 0.0f && x < __builtin_inff(); }

extern "C" int wdgs_tsdf_volume_create(wdgs_device* dev, const float* origin, float voxel_size, uint32_t nx, uint32_t ny, uint32_t nz, float truncation, float max_weight,
                                       uint32_t colour, wdgs_tsdf_volume** out) {
    WDGS_REQUIRE(dev && origin && out, WDGS_E_INVALID, "wdgs_tsdf_volume_create: null argument");
    WDGS_REQUIRE(nx >= 2u && ny >= 2u && nz >= 2u, WDGS_E_INVALID, "wdgs_tsdf_volume_create: every dimension must be at least 2 (got %u x %u x %u)", nx, ny, nz);
    // (<= 12 triangles per cell: 12 * 2^28 < 2^32, so neither the u32 scan nor its total can overflow)
    WDGS_REQUIRE((uint64_t)nx * ny <= (1ull << 28) && (uint64_t)nx * ny * nz <= (1ull << 28), WDGS_E_INVALID,
                 "wdgs_tsdf_volume_create: %u x %u x %u voxels exceed 2^28", nx, ny, nz);
    WDGS_REQUIRE(positive_finite(voxel_size) && positive_finite(truncation), WDGS_E_INVALID,
                 "wdgs_tsdf_volume_create: voxel_size and truncation must be positive and finite (got %g, %g)", (double)voxel_size, (double)truncation);
    WDGS_REQUIRE(max_weight >= 1.0f, WDGS_E_INVALID, "wdgs_tsdf_volume_create: max_weight must be at least 1 (got %g)", (double)max_weight);
    WDGS_REQUIRE(std::isfinite(origin[0]) && std::isfinite(origin[1]) && std::isfinite(origin[2]), WDGS_E_INVALID, "wdgs_tsdf_volume_create: the origin must be finite");
    WDGS_REQUIRE(!dev->capturing, WDGS_E_STATE, "wdgs_tsdf_volume_create while recording a command buffer");
    auto v = std::make_unique<wdgs_tsdf_volume>();
    v->dev = dev;
    for (int a = 0; a < 3; a++) v->origin[a] = origin[a];
    v->voxel_size = voxel_size;
    v->truncation = truncation;
    v->max_weight = max_weight;
    v->dims[0] = nx; v->dims[1] = ny; v->dims[2] = nz;
    v->voxels = (size_t)nx * ny * nz;
    v->cells = (nx - 1u) * (ny - 1u) * (nz - 1u);
    WDGS_TRY(v->tsdf.alloc(v->voxels, false, dev->stream));
    WDGS_TRY(v->weight.alloc(v->voxels, false, dev->stream));
    if (colour) WDGS_TRY(v->rgb.alloc(3u * v->voxels, false, dev->stream));
    WDGS_TRY(v->counts.alloc(v->cells, true, dev->stream));
    WDGS_TRY(v->offsets.alloc(v->cells, true, dev->stream));
    WDGS_TRY(v->total.alloc(1, true, dev->stream));
    WDGS_TRY(scan_scratch_create(&v->scan, v->cells));
    WDGS_TRY(launch_tsdf_reset(dev, v->voxels, v->tsdf, v->weight, v->rgb));
    *out = v.release();
    return WDGS_OK;
}

extern "C" int wdgs_tsdf_volume_destroy(wdgs_tsdf_volume* vol) {
    if (!vol) return WDGS_OK;
    if (wdgs_device_alive(vol->dev) && !vol->dev->capturing) (void)wdgs_sync_lanes(vol->dev);
    delete vol;
    return WDGS_OK;
}

extern "C" int wdgs_tsdf_volume_reset(wdgs_tsdf_volume* vol) {
    WDGS_REQUIRE(vol, WDGS_E_INVALID, "wdgs_tsdf_volume_reset: null volume");
    vol->generation++;
    return launch_tsdf_reset(vol->dev, vol->voxels, vol->tsdf, vol->weight, vol->rgb);
}

extern "C" int wdgs_tsdf_volume_get_tsdf(wdgs_tsdf_volume* vol, void** f32_dev) {
    WDGS_REQUIRE(vol && f32_dev, WDGS_E_INVALID, "wdgs_tsdf_volume_get_tsdf: null argument");
    vol->generation++;   // the host may write through the pointer
    *f32_dev = vol->tsdf;
    return WDGS_OK;
}
extern "C" int wdgs_tsdf_volume_get_weight(wdgs_tsdf_volume* vol, void** f32_dev) {
    WDGS_REQUIRE(vol && f32_dev, WDGS_E_INVALID, "wdgs_tsdf_volume_get_weight: null argument");
    vol->generation++;
    *f32_dev = vol->weight;
    return WDGS_OK;
}
extern "C" int wdgs_tsdf_volume_get_rgb(wdgs_tsdf_volume* vol, void** f32x3_dev) {
    WDGS_REQUIRE(vol && f32x3_dev, WDGS_E_INVALID, "wdgs_tsdf_volume_get_rgb: null argument");
    WDGS_REQUIRE(vol->rgb, WDGS_E_STATE, "TSDFVolume: the volume was created without colour");
    vol->generation++;
    *f32x3_dev = vol->rgb;
    return WDGS_OK;
}
extern "C" int wdgs_tsdf_volume_get_dims(const wdgs_tsdf_volume* vol, uint32_t* dims3) {
    WDGS_REQUIRE(vol && dims3, WDGS_E_INVALID, "wdgs_tsdf_volume_get_dims: null argument");
    for (int a = 0; a < 3; a++) dims3[a] = vol->dims[a];
    return WDGS_OK;
}

extern "C" int wdgs_tsdf_volume_integrate(wdgs_tsdf_volume* vol, const void* depth_f32_dev, const void* weight_sum_f32_dev, const void* colour_rgba8_dev, uint32_t width,
                                          uint32_t height, const void* camera_dev, float min_weight_sum) {
    WDGS_REQUIRE(vol && depth_f32_dev && camera_dev, WDGS_E_INVALID, "wdgs_tsdf_volume_integrate: null argument");
    WDGS_REQUIRE(width > 0 && height > 0 && (uint64_t)width * height <= 0x7FFFFFFFull, WDGS_E_INVALID, "wdgs_tsdf_volume_integrate: bad image size %ux%u", width, height);
    WDGS_REQUIRE(!colour_rgba8_dev || vol->rgb, WDGS_E_STATE, "TSDFVolume.integrate: colour given to a volume created without colour");
    wdgs_device* d = vol->dev;
    // The block lives on the device.  An eager call reads its two size floats back (one 8-byte copy and a wait) and refuses a disagreement; a recorded call cannot
    // wait, and there the kernel itself compares them and writes nothing when they disagree.
    if (!d->capturing) {
        float size[2] = {0.f, 0.f};
        WDGS_CHECK_HIP(hipMemcpyAsync(size, static_cast<const float*>(camera_dev) + 64, sizeof(size), hipMemcpyDeviceToHost, d->stream));
        WDGS_CHECK_HIP(hipStreamSynchronize(d->stream));
        WDGS_REQUIRE(size[0] == (float)width && size[1] == (float)height, WDGS_E_STATE, "TSDFVolume.integrate: the image is %ux%u, the camera block's %gx%g", width, height,
                     (double)size[0], (double)size[1]);
    }
    vol->generation++;
    return launch_tsdf_integrate(d, vol->origin, vol->voxel_size, vol->dims, vol->truncation, vol->max_weight, static_cast<const float*>(camera_dev),
                                 static_cast<const float*>(depth_f32_dev), static_cast<const float*>(weight_sum_f32_dev), static_cast<const u32*>(colour_rgba8_dev), width,
                                 height, min_weight_sum, vol->tsdf, vol->weight, vol->rgb);
}

extern "C" int wdgs_tsdf_volume_count_triangles(wdgs_tsdf_volume* vol, float min_weight, uint32_t* total) {
    WDGS_REQUIRE(vol && total, WDGS_E_INVALID, "wdgs_tsdf_volume_count_triangles: null argument");
    WDGS_REQUIRE(positive_finite(min_weight), WDGS_E_INVALID, "wdgs_tsdf_volume_count_triangles: min_weight must be positive and finite (got %g)", (double)min_weight);
    wdgs_device* d = vol->dev;
    WDGS_REQUIRE(!d->capturing, WDGS_E_STATE, "TSDFVolume.countTriangles waits for its total and cannot be recorded into a command buffer");
    vol->counted_generation = 0;
    WDGS_TRY(launch_tsdf_count(d, vol->origin, vol->voxel_size, vol->dims, vol->tsdf, vol->weight, min_weight, vol->counts));
    WDGS_TRY(scan_exclusive_u32(d, &vol->scan, vol->counts, vol->offsets, vol->cells, vol->total));
    u32 n = 0;
    WDGS_CHECK_HIP(hipMemcpyAsync(&n, vol->total, sizeof(u32), hipMemcpyDeviceToHost, d->stream));
    WDGS_CHECK_HIP(wdgs_sync_lanes(d));
    vol->counted_total = n;
    vol->counted_min_weight = min_weight;
    vol->counted_generation = vol->generation;
    *total = n;
    return WDGS_OK;
}

extern "C" int wdgs_tsdf_volume_emit_triangles(wdgs_tsdf_volume* vol, void* positions_f32_dev, void* keys_u64_dev, void* colours_rgba8_dev, uint32_t capacity_triangles) {
    WDGS_REQUIRE(vol, WDGS_E_INVALID, "wdgs_tsdf_volume_emit_triangles: null volume");
    WDGS_REQUIRE(vol->counted_generation != 0, WDGS_E_STATE, "TSDFVolume.emitTriangles: no countTriangles precedes it");
    WDGS_REQUIRE(vol->counted_generation == vol->generation, WDGS_E_STATE,
                 "TSDFVolume.emitTriangles: the volume was integrated, reset or handed out for writing since countTriangles (count again)");
    WDGS_REQUIRE(!colours_rgba8_dev || vol->rgb, WDGS_E_STATE, "TSDFVolume.emitTriangles: vertex colours asked of a volume created without colour");
    WDGS_REQUIRE(capacity_triangles >= vol->counted_total, WDGS_E_CAPACITY, "TSDFVolume.emitTriangles: %u triangles, room for %u", vol->counted_total, capacity_triangles);
    if (vol->counted_total == 0) return WDGS_OK;
    WDGS_REQUIRE(positions_f32_dev, WDGS_E_INVALID, "wdgs_tsdf_volume_emit_triangles: null positions");
    WDGS_REQUIRE(((uintptr_t)keys_u64_dev & 7u) == 0u && ((uintptr_t)positions_f32_dev & 3u) == 0u && ((uintptr_t)colours_rgba8_dev & 3u) == 0u, WDGS_E_INVALID,
                 "wdgs_tsdf_volume_emit_triangles: misaligned output");
    return launch_tsdf_emit(vol->dev, vol->origin, vol->voxel_size, vol->dims, vol->tsdf, vol->weight, colours_rgba8_dev ? vol->rgb.get() : nullptr,
                            vol->counted_min_weight, vol->counts, vol->offsets, static_cast<float*>(positions_f32_dev), static_cast<unsigned long long*>(keys_u64_dev),
                            static_cast<u32*>(colours_rgba8_dev));
}
