// Welding a triangle soup on the device: the C ABI object (include/webdgs.h) over the stable u64 key sort of keysort.hip (no counterpart
// in the reference, which renders colour only).
//
// S = 3F slots carry keys u64[S]; the distinct keys in ascending order are the vertices, every slot's face index is the rank of its key, and a vertex takes
// the position and colour bits of the LOWEST slot that carries its key.  The count sorts, flags the heads of the runs of equal keys and scans the flags; the
// host waits a single time, for V, and reads the plan's pass count with it.  The emit is the sort's gather and waits for nothing.
#include <memory>

#include "launch.h"

struct wdgs_mesh_welder {
    wdgs_device* dev = nullptr;
    KeySort sort;
    bool counted = false;
    const void* keys = nullptr;                  // the caller's, read again by emit when no pass ran
    u32 S = 0, V = 0, passes_run = 0;
};

extern "C" int wdgs_mesh_welder_create(wdgs_device* dev, wdgs_mesh_welder** out) {
    WDGS_REQUIRE(dev && out, WDGS_E_INVALID, "wdgs_mesh_welder_create: null argument");
    WDGS_REQUIRE(!dev->capturing, WDGS_E_STATE, "wdgs_mesh_welder_create while recording a command buffer");
    auto w = std::make_unique<wdgs_mesh_welder>();
    w->dev = dev;
    WDGS_TRY(w->sort.create(dev));
    *out = w.release();
    return WDGS_OK;
}

extern "C" int wdgs_mesh_welder_destroy(wdgs_mesh_welder* w) {
    if (!w) return WDGS_OK;
    if (wdgs_device_alive(w->dev) && !w->dev->capturing) (void)wdgs_sync_lanes(w->dev);
    delete w;
    return WDGS_OK;
}

extern "C" int wdgs_mesh_welder_count(wdgs_mesh_welder* w, const void* keys_u64_dev, uint64_t num_slots, uint32_t* num_vertices) {
    WDGS_REQUIRE(w && num_vertices, WDGS_E_INVALID, "wdgs_mesh_welder_count: null argument");
    w->counted = false;   // (a refused count leaves nothing to emit)
    WDGS_REQUIRE(num_slots < (1ull << 32) && num_slots % 3ull == 0ull, WDGS_E_INVALID, "weldTriangles: %llu slots: not three per triangle, or 2^32 or more",
                 (unsigned long long)num_slots);
    WDGS_REQUIRE(num_slots == 0 || keys_u64_dev, WDGS_E_INVALID, "wdgs_mesh_welder_count: null keys");
    WDGS_REQUIRE(((uintptr_t)keys_u64_dev & 7u) == 0u, WDGS_E_INVALID, "wdgs_mesh_welder_count: misaligned keys");
    wdgs_device* d = w->dev;
    WDGS_REQUIRE(!d->capturing, WDGS_E_STATE, "weldTriangles: the count waits for its vertex count and cannot be recorded into a command buffer");
    *num_vertices = 0;
    const u32 S = (u32)num_slots;
    WDGS_TRY(w->sort.reserve(d, S));
    u32 host[3] = {0u, 0u, 0u};   // the counters' first words: KS_C_TOTAL, KS_C_PASSES (and the final buffer), in one copy
    if (S != 0) {
        WDGS_TRY(w->sort.sort(d, static_cast<const unsigned long long*>(keys_u64_dev), S, w->sort.total()));
        WDGS_CHECK_HIP(hipMemcpyAsync(host, w->sort.counters, sizeof(host), hipMemcpyDeviceToHost, d->stream));
        WDGS_CHECK_HIP(wdgs_sync_lanes(d));
    }
    w->keys = keys_u64_dev;
    w->S = S;
    w->V = host[KS_C_TOTAL];
    w->passes_run = host[KS_C_PASSES];
    w->counted = true;
    *num_vertices = w->V;
    return WDGS_OK;
}

extern "C" int wdgs_mesh_welder_emit(wdgs_mesh_welder* w, const void* keys_u64_dev, uint64_t num_slots, const void* positions_f32_dev, const void* colours_rgba8_dev,
                                     void* keys_out_u64_dev, void* vertices_out_f32_dev, void* colours_out_rgba8_dev, void* faces_out_u32_dev, uint32_t capacity_vertices) {
    WDGS_REQUIRE(w, WDGS_E_INVALID, "wdgs_mesh_welder_emit: null argument");
    WDGS_REQUIRE(w->counted && keys_u64_dev == w->keys && num_slots == (uint64_t)w->S, WDGS_E_STATE, "weldTriangles: no count of these keys precedes the emit");
    WDGS_REQUIRE(capacity_vertices >= w->V, WDGS_E_CAPACITY, "weldTriangles: %u vertices, room for %u", w->V, capacity_vertices);
    WDGS_REQUIRE((positions_f32_dev == nullptr) == (vertices_out_f32_dev == nullptr), WDGS_E_INVALID, "wdgs_mesh_welder_emit: positions need both an input and an output");
    WDGS_REQUIRE((colours_rgba8_dev == nullptr) == (colours_out_rgba8_dev == nullptr), WDGS_E_INVALID, "wdgs_mesh_welder_emit: colours need both an input and an output");
    WDGS_REQUIRE(w->S == 0 || faces_out_u32_dev, WDGS_E_INVALID, "wdgs_mesh_welder_emit: null faces output");
    WDGS_REQUIRE((((uintptr_t)positions_f32_dev | (uintptr_t)colours_rgba8_dev | (uintptr_t)vertices_out_f32_dev | (uintptr_t)colours_out_rgba8_dev | (uintptr_t)faces_out_u32_dev) & 3u) == 0u &&
                     ((uintptr_t)keys_out_u64_dev & 7u) == 0u,
                 WDGS_E_INVALID, "wdgs_mesh_welder_emit: misaligned buffer");
    if (w->S == 0) return WDGS_OK;
    return w->sort.emit(w->dev, static_cast<const unsigned long long*>(keys_u64_dev), w->S, static_cast<u32*>(faces_out_u32_dev),
                        static_cast<unsigned long long*>(keys_out_u64_dev), static_cast<const u32*>(colours_rgba8_dev), static_cast<u32*>(colours_out_rgba8_dev),
                        static_cast<const float*>(positions_f32_dev), static_cast<float*>(vertices_out_f32_dev));
}

extern "C" int wdgs_mesh_welder_stats(const wdgs_mesh_welder* w, uint32_t* passes_run, uint32_t* passes_skipped, uint32_t* num_vertices, uint32_t* num_slots) {
    WDGS_REQUIRE(w, WDGS_E_INVALID, "wdgs_mesh_welder_stats: null argument");
    WDGS_REQUIRE(w->counted, WDGS_E_STATE, "weldTriangles: no count precedes the read of its statistics");
    if (passes_run) *passes_run = w->passes_run;
    if (passes_skipped) *passes_skipped = KS_PASSES - w->passes_run;
    if (num_vertices) *num_vertices = w->V;
    if (num_slots) *num_slots = w->S;
    return WDGS_OK;
}
