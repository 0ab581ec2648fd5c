// Mesh connected components and small-component removal (no counterpart in the reference, which renders colour only).
//
// An indexed mesh faces u32[F][3] over V vertices is cut into the classes of "some valid face names both vertices", taken transitively; a class with a valid
// face is a component, its representative its lowest vertex, and components are numbered in ascending order of representative.  Everything is integer work,
// and every output is a function of the input alone: the union-find below always links the LARGER root under the SMALLER, so the root a set ends with is its
// lowest index whatever order the threads ran in, and everything behind it (numbers by a scan over the roots, sizes by integer atomics, compaction by
// flag / scan / emit) has no order to depend on.  tests/meshclean_ref.py restates it in numpy and the GPU tests compare bytes.
//
// The hook and the flatten kernel are the only places where threads of one launch read what others of the same launch write.  There every access to
// parent[] is a relaxed agent-scope atomic (an L2-served load, a store that goes through, a read-modify-write at the memory side); nothing waits for
// anything: parent[v] <= v at all times, so every walk strictly descends and ends by itself.  Section 16 holds the argument that a stale read is harmless.
// All other kernels read what earlier launches wrote, with plain loads.
#include <algorithm>
#include <memory>
#include <vector>

#include "launch.h"

namespace {

constexpr u32 NO_COMPONENT = 0xFFFFFFFFu;
constexpr u32 MC_THREADS = 256;

__device__ __forceinline__ u32 uf_ld(const u32* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void uf_st(u32* p, u32 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ u32 uf_min(u32* p, u32 v) { return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ u32 uf_cas(u32* p, u32 expected, u32 desired) {
    (void)__hip_atomic_compare_exchange_strong(p, &expected, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return expected;   // the value found: `expected` itself when the exchange took place
}

// The root of x's tree: walks parent[] down until parent[r] == r, pointing every vertex passed at its grandparent (path splitting, as uf_unite does).
__device__ __forceinline__ u32 uf_find(u32* parent, u32 x) {
    u32 p = uf_ld(parent + x);
    while (p != x) {
        const u32 g = uf_ld(parent + p);
        if (g != p) (void)uf_min(parent + x, g);
        x = p;
        p = g;
    }
    return x;
}

// Joins the sets of a and b.  The walk stands on one vertex of each set and always advances the LARGER of the two (Rem's scheme): it ends when both stand on
// the same vertex -- one set already -- or when the larger is a root, which is then linked under the smaller by a CAS that succeeds only while it still IS a
// root; when it is not, the walk goes on from the parent the CAS found there.  The smaller vertex need not be a root: hanging a root under an inner vertex of
// the other set joins the sets all the same and keeps parent[v] <= v.  Neither walk has to reach its set's root, so a union of neighbours in a long chain costs
// a few steps however deep the chain is.  Every vertex passed is pointed at its grandparent (path splitting) with an atomic MIN, so parent[] only ever
// decreases and a slower thread can never undo a shorter path.
__device__ __forceinline__ void uf_unite(u32* parent, u32 a, u32 b) {
    u32 u = max(a, b), v = min(a, b);
    while (u != v) {
        const u32 p = uf_ld(parent + u);
        if (p == u) {
            const u32 found = uf_cas(parent + u, u, v);
            if (found == u) return;
            u = found;
        } else {
            const u32 g = uf_ld(parent + p);
            if (g != p) (void)uf_min(parent + u, g);
            u = p;
        }
        if (u < v) { const u32 t = u; u = v; v = t; }
    }
}

__global__ __launch_bounds__(MC_THREADS) void mc_init_kernel(u32* __restrict__ parent, u32 V) {
    const u32 v = blockIdx.x * MC_THREADS + threadIdx.x;
    if (v < V) parent[v] = v;
}

// One thread per face: a valid face unites (a, b) and (a, c); the invalid ones are counted, one atomic per wave.
__global__ __launch_bounds__(MC_THREADS) void mc_hook_kernel(const u32* __restrict__ faces, u32 F, u32 V, u32* parent, u32* __restrict__ invalid_faces) {
    const u32 t = blockIdx.x * MC_THREADS + threadIdx.x;
    bool invalid = false;
    if (t < F) {
        const u32 a = faces[3u * (size_t)t], b = faces[3u * (size_t)t + 1u], c = faces[3u * (size_t)t + 2u];
        if (a < V && b < V && c < V) {
            if (a != b) uf_unite(parent, a, b);
            if (a != c) uf_unite(parent, a, c);
        } else {
            invalid = true;
        }
    }
    const unsigned long long m = __ballot(invalid);
    if (m != 0ull && (threadIdx.x & 63u) == (u32)(__ffsll((long long)m) - 1)) atomicAdd(invalid_faces, (u32)__popcll(m));
}

// parent[v] = the root of v.  Roots are final here (no link is made after the hook launch), so the walk ends at the set's lowest index; the threads of this
// launch shorten each other's paths meanwhile (a chain of depth n is flat after about log2 n steps each), hence the atomic accesses, and whatever a walk
// reads is an ancestor of where it stands.
__global__ __launch_bounds__(MC_THREADS) void mc_flatten_kernel(u32* parent, u32 V) {
    const u32 v = blockIdx.x * MC_THREADS + threadIdx.x;
    if (v >= V) return;
    uf_st(parent + v, uf_find(parent, v));
}

// used[r] = 1 for the root r of every valid face (equal stores; `used` was cleared).  A vertex is named by a valid face exactly when its root is used: a vertex
// that none names was never united with anything and is its own, unused, root.
__global__ __launch_bounds__(MC_THREADS) void mc_mark_kernel(const u32* __restrict__ faces, u32 F, u32 V, const u32* __restrict__ root, u32* __restrict__ used) {
    const u32 t = blockIdx.x * MC_THREADS + threadIdx.x;
    if (t >= F) return;
    const u32 a = faces[3u * (size_t)t], b = faces[3u * (size_t)t + 1u], c = faces[3u * (size_t)t + 2u];
    if (a < V && b < V && c < V) used[root[a]] = 1u;
}

// Sizes by integer atomics, aggregated before they reach memory: on a fused mesh nearly every face of a wave, and of the next wave, lies in one component, and
// one add per face -- or per wave -- onto that component's word is a queue at one address.  A wave labels MC_LABEL_ITEMS chunks of 64 consecutive elements and
// carries a run { key, count }: per chunk the key of its first lane that has one is matched across the wave (ballot) and joins the run if it is the run's key,
// else the run is flushed with ONE add and a new one begins; up to three more distinct keys of the chunk get one add each, what is left one add per lane.
// Every lane runs every ballot and shuffle, run_key and run_count are uniform, and the loops' exits are uniform.
constexpr u32 MC_LABEL_ITEMS = 8;

__device__ __forceinline__ void wave_run_flush(u32* __restrict__ counts, u32 run_key, u32 run_count) {
    if (run_count != 0u && (threadIdx.x & 63u) == 0u) atomicAdd(counts + run_key, run_count);
}

__device__ __forceinline__ void wave_count(u32* __restrict__ counts, u32 key, u32& run_key, u32& run_count) {
    const u32 lane = threadIdx.x & 63u;
    bool pending = key != NO_COMPONENT;
    for (u32 round = 0; round < 4u; round++) {
        const unsigned long long m = __ballot(pending);
        if (m == 0ull) return;
        const u32 leader = (u32)(__ffsll((long long)m) - 1);
        const u32 k = (u32)__shfl((int)key, (int)leader, 64);
        const bool same = pending && key == k;
        const u32 n = (u32)__popcll(__ballot(same));
        if (round == 0u) {
            if (k == run_key) {
                run_count += n;
            } else {
                wave_run_flush(counts, run_key, run_count);
                run_key = k;
                run_count = n;
            }
        } else if (lane == leader) {
            atomicAdd(counts + k, n);
        }
        pending = pending && !same;
    }
    if (pending) atomicAdd(counts + key, 1u);
}

// Element i of chunk `item` of the calling wave: waves own MC_LABEL_ITEMS * 64 consecutive elements each
__device__ __forceinline__ size_t label_element(u32 item) {
    const size_t wave = ((size_t)blockIdx.x * MC_THREADS + threadIdx.x) >> 6;
    return (wave * MC_LABEL_ITEMS + item) * 64u + (threadIdx.x & 63u);
}

// number: the exclusive scan of used.  vertexComponent[v] = number[root[v]] where that root is used, and the components' vertex counts.
__global__ __launch_bounds__(MC_THREADS) void mc_label_vertices_kernel(u32 V, const u32* __restrict__ root, const u32* __restrict__ used, const u32* __restrict__ number,
                                                                       u32* __restrict__ vertex_component, u32* __restrict__ vertex_counts) {
    u32 run_key = NO_COMPONENT, run_count = 0u;
    for (u32 item = 0; item < MC_LABEL_ITEMS; item++) {
        const size_t v = label_element(item);
        u32 comp = NO_COMPONENT;
        if (v < V) {
            const u32 r = root[v];
            if (used[r] != 0u) comp = number[r];
            vertex_component[v] = comp;
        }
        wave_count(vertex_counts, comp, run_key, run_count);
    }
    wave_run_flush(vertex_counts, run_key, run_count);
}

__global__ __launch_bounds__(MC_THREADS) void mc_label_faces_kernel(const u32* __restrict__ faces, u32 F, u32 V, const u32* __restrict__ root, const u32* __restrict__ number,
                                                                    u32* __restrict__ face_component, u32* __restrict__ triangle_counts) {
    u32 run_key = NO_COMPONENT, run_count = 0u;
    for (u32 item = 0; item < MC_LABEL_ITEMS; item++) {
        const size_t t = label_element(item);
        u32 comp = NO_COMPONENT;
        if (t < F) {
            const u32 a = faces[3u * t], b = faces[3u * t + 1u], c = faces[3u * t + 2u];
            if (a < V && b < V && c < V) comp = number[root[a]];
            face_component[t] = comp;
        }
        wave_count(triangle_counts, comp, run_key, run_count);
    }
    wave_run_flush(triangle_counts, run_key, run_count);
}

// flags[i] = 1 where element i's component is kept (keep: u32[C], 0 or 1)
__global__ __launch_bounds__(MC_THREADS) void mc_keep_flags_kernel(u32 n, const u32* __restrict__ component, const u32* __restrict__ keep, u32 C, u32* __restrict__ flags) {
    const u32 i = blockIdx.x * MC_THREADS + threadIdx.x;
    if (i >= n) return;
    const u32 c = component[i];
    flags[i] = (c < C && keep[c] != 0u) ? 1u : 0u;
}

// A kept vertex v goes to slot offsets[v]: its position (both nullable together) and its old index
__global__ __launch_bounds__(MC_THREADS) void mc_emit_vertices_kernel(u32 V, const u32* __restrict__ flags, const u32* __restrict__ offsets, const float* __restrict__ positions,
                                                                      float* __restrict__ positions_out, u32* __restrict__ vertex_map) {
    const u32 v = blockIdx.x * MC_THREADS + threadIdx.x;
    if (v >= V || flags[v] == 0u) return;
    const u32 s = offsets[v];
    if (positions_out) {
#pragma unroll
        for (u32 a = 0; a < 3u; a++) positions_out[3u * (size_t)s + a] = positions[3u * (size_t)v + a];
    }
    if (vertex_map) vertex_map[s] = v;
}

// A kept face t goes to slot offsets[t] with its corners renumbered.  (A face array rewritten behind the library's back since the labelling may name any
// vertex now: an index that is no vertex, or no kept one, is written as 0xFFFFFFFF and nothing outside the arrays is read.)
__global__ __launch_bounds__(MC_THREADS) void mc_emit_faces_kernel(const u32* __restrict__ faces, u32 F, u32 V, const u32* __restrict__ flags, const u32* __restrict__ offsets,
                                                                   const u32* __restrict__ vertex_flags, const u32* __restrict__ vertex_offsets, u32* __restrict__ faces_out,
                                                                   u32* __restrict__ face_map) {
    const u32 t = blockIdx.x * MC_THREADS + threadIdx.x;
    if (t >= F || flags[t] == 0u) return;
    const u32 s = offsets[t];
#pragma unroll
    for (u32 a = 0; a < 3u; a++) {
        const u32 v = faces[3u * (size_t)t + a];
        faces_out[3u * (size_t)s + a] = (v < V && vertex_flags[v] != 0u) ? vertex_offsets[v] : NO_COMPONENT;
    }
    if (face_map) face_map[s] = t;
}

inline dim3 mc_grid(u32 n) { return dim3(ceil_div(n, MC_THREADS)); }

}  // namespace

// ---------------------------------------------------------------- launchers
int launch_mesh_hook(wdgs_device* dev, const u32* faces, u32 F, u32 V, u32* parent, u32* invalid_faces) {
    WDGS_CHECK_HIP(hipMemsetAsync(invalid_faces, 0, 4, dev->stream));
    if (V != 0) WDGS_LAUNCH(dev, "mesh_init", mc_init_kernel, mc_grid(V), dim3(MC_THREADS), 0, parent, V);
    if (F != 0) WDGS_LAUNCH(dev, "mesh_hook", mc_hook_kernel, mc_grid(F), dim3(MC_THREADS), 0, faces, F, V, parent, invalid_faces);
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

int launch_mesh_roots(wdgs_device* dev, const u32* faces, u32 F, u32 V, u32* parent, u32* used) {
    if (V == 0) return WDGS_OK;
    WDGS_CHECK_HIP(hipMemsetAsync(used, 0, 4 * (size_t)V, dev->stream));
    WDGS_LAUNCH(dev, "mesh_flatten", mc_flatten_kernel, mc_grid(V), dim3(MC_THREADS), 0, parent, V);
    if (F != 0) WDGS_LAUNCH(dev, "mesh_mark", mc_mark_kernel, mc_grid(F), dim3(MC_THREADS), 0, faces, F, V, (const u32*)parent, used);
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

int launch_mesh_label(wdgs_device* dev, const u32* faces, u32 F, u32 V, const u32* root, const u32* used, const u32* number, u32* vertex_component, u32* face_component,
                      u32* vertex_counts, u32* triangle_counts) {
    if (V != 0)
        WDGS_LAUNCH(dev, "mesh_label_vertices", mc_label_vertices_kernel, dim3(ceil_div(V, MC_THREADS * MC_LABEL_ITEMS)), dim3(MC_THREADS), 0, V, root, used, number, vertex_component, vertex_counts);
    if (F != 0)
        WDGS_LAUNCH(dev, "mesh_label_faces", mc_label_faces_kernel, dim3(ceil_div(F, MC_THREADS * MC_LABEL_ITEMS)), dim3(MC_THREADS), 0, faces, F, V, root, number, face_component, triangle_counts);
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

int launch_mesh_keep_flags(wdgs_device* dev, u32 n, const u32* component, const u32* keep, u32 C, u32* flags) {
    if (n == 0) return WDGS_OK;
    WDGS_LAUNCH(dev, "mesh_keep_flags", mc_keep_flags_kernel, mc_grid(n), dim3(MC_THREADS), 0, n, component, keep, C, flags);
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

int launch_mesh_emit(wdgs_device* dev, const u32* faces, u32 F, u32 V, const u32* vertex_flags, const u32* vertex_offsets, const u32* face_flags, const u32* face_offsets,
                     const float* positions, float* positions_out, u32* vertex_map, u32* faces_out, u32* face_map) {
    if (V != 0 && (positions_out || vertex_map))
        WDGS_LAUNCH(dev, "mesh_emit_vertices", mc_emit_vertices_kernel, mc_grid(V), dim3(MC_THREADS), 0, V, vertex_flags, vertex_offsets, positions, positions_out, vertex_map);
    if (F != 0)
        WDGS_LAUNCH(dev, "mesh_emit_faces", mc_emit_faces_kernel, mc_grid(F), dim3(MC_THREADS), 0, faces, F, V, face_flags, face_offsets, vertex_flags, vertex_offsets,
                    faces_out, face_map);
    WDGS_CHECK_HIP(hipGetLastError());
    return WDGS_OK;
}

// ---------------------------------------------------------------- the C ABI object (include/webdgs.h)
struct wdgs_mesh_components {
    wdgs_device* dev = nullptr;
    DevMem<u32> parent;                    // [V]: the union-find, then every vertex's root
    DevMem<u32> used, number;              // [V]: root flags and their scan; after a select, the kept-vertex flags and their scan
    DevMem<u32> vertex_component;          // [V]
    DevMem<u32> face_component;            // [F]
    DevMem<u32> face_flags, face_offsets;  // [F]: a select's kept-face flags and their scan
    DevMem<u32> triangles, vertices;       // [C]: the components' sizes
    DevMem<u32> keep;                      // [C]: the selection
    DevMem<u32> counters;                  // C, invalid faces, kept vertices, kept faces
    ScanScratch scan;
    u32 capacity_v = 0, capacity_f = 0, capacity_c = 0, capacity_keep = 0, capacity_scan = 0;
    bool labelled = false, selected = false;
    const void* faces = nullptr;           // the caller's, read again by compact
    u32 V = 0, F = 0, C = 0, invalid = 0, kept_v = 0, kept_f = 0;
};

extern "C" int wdgs_mesh_components_create(wdgs_device* dev, wdgs_mesh_components** out) {
    WDGS_REQUIRE(dev && out, WDGS_E_INVALID, "wdgs_mesh_components_create: null argument");
    WDGS_REQUIRE(!dev->capturing, WDGS_E_STATE, "wdgs_mesh_components_create while recording a command buffer");
    auto c = std::make_unique<wdgs_mesh_components>();
    c->dev = dev;
    WDGS_TRY(c->counters.alloc(4, true, dev->stream));
    *out = c.release();
    return WDGS_OK;
}

extern "C" int wdgs_mesh_components_destroy(wdgs_mesh_components* c) {
    if (!c) return WDGS_OK;
    if (wdgs_device_alive(c->dev) && !c->dev->capturing) (void)wdgs_sync_lanes(c->dev);
    delete c;
    return WDGS_OK;
}

extern "C" int wdgs_mesh_components_label(wdgs_mesh_components* c, const void* faces_u32_dev, uint32_t num_faces, uint32_t num_vertices, uint32_t* num_components,
                                          uint32_t* invalid_faces) {
    WDGS_REQUIRE(c && num_components && invalid_faces, WDGS_E_INVALID, "wdgs_mesh_components_label: null argument");
    c->labelled = c->selected = false;   // (a refused labelling leaves nothing to read or compact)
    WDGS_REQUIRE(num_faces == 0 || faces_u32_dev, WDGS_E_INVALID, "wdgs_mesh_components_label: null faces");
    WDGS_REQUIRE(num_faces < (1u << 31) && num_vertices < (1u << 31), WDGS_E_INVALID, "meshComponents: %u faces over %u vertices, 2^31 or more", num_faces, num_vertices);
    WDGS_REQUIRE(((uintptr_t)faces_u32_dev & 3u) == 0u, WDGS_E_INVALID, "wdgs_mesh_components_label: misaligned faces");
    wdgs_device* d = c->dev;
    WDGS_REQUIRE(!d->capturing, WDGS_E_STATE, "meshComponents: the labelling waits for its component count and cannot be recorded into a command buffer");
    *num_components = *invalid_faces = 0;
    const u32 V = num_vertices, F = num_faces;
    if (V > c->capacity_v || F > c->capacity_f || std::max(V, F) > c->capacity_scan) {
        WDGS_CHECK_HIP(wdgs_sync_lanes(d));   // (nothing in flight may still read the blocks given back)
        if (V > c->capacity_v) {
            c->capacity_v = 0;
            WDGS_TRY(c->parent.alloc(V, false, d->stream));
            WDGS_TRY(c->used.alloc(V, false, d->stream));
            WDGS_TRY(c->number.alloc(V, false, d->stream));
            WDGS_TRY(c->vertex_component.alloc(V, false, d->stream));
            c->capacity_v = V;
        }
        if (F > c->capacity_f) {
            c->capacity_f = 0;
            WDGS_TRY(c->face_component.alloc(F, false, d->stream));
            WDGS_TRY(c->face_flags.alloc(F, false, d->stream));
            WDGS_TRY(c->face_offsets.alloc(F, false, d->stream));
            c->capacity_f = F;
        }
        if (std::max(V, F) > c->capacity_scan) {
            c->capacity_scan = 0;
            WDGS_TRY(scan_scratch_create(&c->scan, std::max(V, F)));
            c->capacity_scan = std::max(V, F);
        }
    }
    const u32* faces = static_cast<const u32*>(faces_u32_dev);
    WDGS_TRY(launch_mesh_hook(d, faces, F, V, c->parent, c->counters + 1));
    WDGS_TRY(launch_mesh_roots(d, faces, F, V, c->parent, c->used));
    WDGS_TRY(scan_exclusive_u32(d, &c->scan, c->used, c->number, V, c->counters));
    u32 host[2] = {0u, 0u};
    WDGS_CHECK_HIP(hipMemcpyAsync(host, c->counters, sizeof(host), hipMemcpyDeviceToHost, d->stream));
    WDGS_CHECK_HIP(wdgs_sync_lanes(d));
    const u32 C = host[0];
    if (C > c->capacity_c) {
        c->capacity_c = 0;
        WDGS_TRY(c->triangles.alloc(C, false, d->stream));
        WDGS_TRY(c->vertices.alloc(C, false, d->stream));
        c->capacity_c = C;
    }
    if (C != 0) {
        WDGS_CHECK_HIP(hipMemsetAsync(c->triangles, 0, 4 * (size_t)C, d->stream));
        WDGS_CHECK_HIP(hipMemsetAsync(c->vertices, 0, 4 * (size_t)C, d->stream));
    }
    WDGS_TRY(launch_mesh_label(d, faces, F, V, c->parent, c->used, c->number, c->vertex_component, c->face_component, c->vertices, c->triangles));
    c->faces = faces_u32_dev;
    c->V = V;
    c->F = F;
    c->C = C;
    c->invalid = host[1];
    c->labelled = true;
    *num_components = C;
    *invalid_faces = host[1];
    return WDGS_OK;
}

extern "C" int wdgs_mesh_components_get(wdgs_mesh_components* c, void** face_component_u32_dev, void** vertex_component_u32_dev, void** triangles_u32_dev,
                                        void** vertices_u32_dev) {
    WDGS_REQUIRE(c, WDGS_E_INVALID, "wdgs_mesh_components_get: null argument");
    WDGS_REQUIRE(c->labelled, WDGS_E_STATE, "meshComponents: no labelling precedes the read");
    if (face_component_u32_dev) *face_component_u32_dev = c->F ? c->face_component.get() : nullptr;
    if (vertex_component_u32_dev) *vertex_component_u32_dev = c->V ? c->vertex_component.get() : nullptr;
    if (triangles_u32_dev) *triangles_u32_dev = c->C ? c->triangles.get() : nullptr;
    if (vertices_u32_dev) *vertices_u32_dev = c->C ? c->vertices.get() : nullptr;
    return WDGS_OK;
}

extern "C" int wdgs_mesh_components_select(wdgs_mesh_components* c, const uint8_t* keep_host, uint32_t num_components, uint32_t* kept_vertices, uint32_t* kept_faces) {
    WDGS_REQUIRE(c && kept_vertices && kept_faces, WDGS_E_INVALID, "wdgs_mesh_components_select: null argument");
    WDGS_REQUIRE(c->labelled, WDGS_E_STATE, "removeSmallComponents: no labelling precedes the selection");
    WDGS_REQUIRE(num_components == c->C, WDGS_E_INVALID, "removeSmallComponents: a selection of %u components for a mesh of %u", num_components, c->C);
    WDGS_REQUIRE(num_components == 0 || keep_host, WDGS_E_INVALID, "wdgs_mesh_components_select: null selection");
    wdgs_device* d = c->dev;
    WDGS_REQUIRE(!d->capturing, WDGS_E_STATE, "removeSmallComponents: the selection waits for its counts and cannot be recorded into a command buffer");
    c->selected = false;
    *kept_vertices = *kept_faces = 0;
    const u32 C = c->C;
    if (C > c->capacity_keep) {
        WDGS_CHECK_HIP(wdgs_sync_lanes(d));
        c->capacity_keep = 0;
        WDGS_TRY(c->keep.alloc(C, false, d->stream));
        c->capacity_keep = C;
    }
    std::vector<u32> words(C);
    for (u32 i = 0; i < C; i++) words[i] = keep_host[i] ? 1u : 0u;
    if (C != 0) WDGS_CHECK_HIP(hipMemcpyAsync(c->keep, words.data(), 4 * (size_t)C, hipMemcpyHostToDevice, d->stream));
    // (the root flags and their scan are not needed after the labelling: their arrays hold the kept-vertex flags and offsets from here on)
    WDGS_TRY(launch_mesh_keep_flags(d, c->V, c->vertex_component, c->keep, C, c->used));
    WDGS_TRY(launch_mesh_keep_flags(d, c->F, c->face_component, c->keep, C, c->face_flags));
    WDGS_TRY(scan_exclusive_u32(d, &c->scan, c->used, c->number, c->V, c->counters + 2));
    WDGS_TRY(scan_exclusive_u32(d, &c->scan, c->face_flags, c->face_offsets, c->F, c->counters + 3));
    u32 host[2] = {0u, 0u};
    WDGS_CHECK_HIP(hipMemcpyAsync(host, c->counters + 2, sizeof(host), hipMemcpyDeviceToHost, d->stream));
    WDGS_CHECK_HIP(wdgs_sync_lanes(d));   // (also: `words` has been read)
    c->kept_v = host[0];
    c->kept_f = host[1];
    c->selected = true;
    *kept_vertices = host[0];
    *kept_faces = host[1];
    return WDGS_OK;
}

extern "C" int wdgs_mesh_components_compact(wdgs_mesh_components* c, const void* vertices_f32_dev, void* vertices_out_f32_dev, void* faces_out_u32_dev,
                                            void* vertex_map_u32_dev, void* face_map_u32_dev, uint32_t capacity_vertices, uint32_t capacity_faces) {
    WDGS_REQUIRE(c, WDGS_E_INVALID, "wdgs_mesh_components_compact: null argument");
    WDGS_REQUIRE(c->labelled && c->selected, WDGS_E_STATE, "removeSmallComponents: no selection precedes the compaction");
    WDGS_REQUIRE(capacity_vertices >= c->kept_v && capacity_faces >= c->kept_f, WDGS_E_CAPACITY, "removeSmallComponents: %u vertices and %u faces, room for %u and %u",
                 c->kept_v, c->kept_f, capacity_vertices, capacity_faces);
    WDGS_REQUIRE((vertices_f32_dev == nullptr) == (vertices_out_f32_dev == nullptr) || c->kept_v == 0, WDGS_E_INVALID,
                 "wdgs_mesh_components_compact: positions need both an input and an output");
    WDGS_REQUIRE(c->kept_f == 0 || faces_out_u32_dev, WDGS_E_INVALID, "wdgs_mesh_components_compact: null faces output");
    WDGS_REQUIRE((((uintptr_t)vertices_f32_dev | (uintptr_t)vertices_out_f32_dev | (uintptr_t)faces_out_u32_dev | (uintptr_t)vertex_map_u32_dev | (uintptr_t)face_map_u32_dev) & 3u) == 0u,
                 WDGS_E_INVALID, "wdgs_mesh_components_compact: misaligned buffer");
    const bool positions = vertices_f32_dev && vertices_out_f32_dev;
    return launch_mesh_emit(c->dev, static_cast<const u32*>(c->faces), c->kept_f ? c->F : 0u, c->kept_v ? c->V : 0u, c->used, c->number, c->face_flags, c->face_offsets,
                            positions ? static_cast<const float*>(vertices_f32_dev) : nullptr, positions ? static_cast<float*>(vertices_out_f32_dev) : nullptr,
                            static_cast<u32*>(vertex_map_u32_dev), static_cast<u32*>(faces_out_u32_dev), static_cast<u32*>(face_map_u32_dev));
}
