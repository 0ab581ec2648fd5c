// C ABI of libwebdgs_hip.so (include/webdgs.h): handle types, ownership, launch sequencing.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <mutex>
#include <map>
#include <memory>
#include <set>
#include <unordered_map>
#include <vector>

#include "launch.h"   // the kernel launchers and scan / sort primitives this file sequences: void* from the C ABI is cast where it meets one
#include "alloc_cache.h"
#include "longlist.h"

static thread_local char g_last_error[512] = "";

// Devices that have been created and not yet destroyed.  Every op keeps a pointer to its device; a host that tears things down
// in the wrong order (an interpreter finalising its objects at exit, say) may call an op's destroy after wdgs_device_destroy.
// Destroy functions therefore ask here before they touch op->dev, and only release memory when the device is already gone.
static std::mutex g_live_mutex;
static std::set<const wdgs_device*> g_live_devices;
bool wdgs_device_alive(const wdgs_device* d) {
    std::lock_guard<std::mutex> lock(g_live_mutex);
    return d && g_live_devices.count(d) != 0;
}
// stream of a live device that is not in the middle of a recording, else nullptr ("nothing to wait for")
static void sync_if_alive(wdgs_device* d) {
    if (wdgs_device_alive(d) && !d->capturing) (void)wdgs_sync_lanes(d);
}

void wdgs_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_last_error, sizeof(g_last_error), fmt, ap);
    va_end(ap);
}

// ---------------------------------------------------------------- device memory
// Freed blocks are kept by size class and handed out again (alloc_cache.h: why, and the per-device epochs that say when a freed block is safe).
// WDGS_ALLOC_CACHE=0: plain hipMalloc / hipFree.  The cache holds at most a quarter of the device's memory; wdgs_device_destroy empties it.
namespace {
struct HipBackend {
    void* malloc(int device, size_t bytes) {
        int cur = 0;
        if (hipGetDevice(&cur) != hipSuccess) return nullptr;
        if (cur != device && hipSetDevice(device) != hipSuccess) return nullptr;
        void* p = nullptr;
        const hipError_t e = hipMalloc(&p, bytes);
        if (cur != device) (void)hipSetDevice(cur);
        if (e != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        return p;
    }
    void free(void* p) { (void)hipFree(p); }
    bool sync(int device) {   // every stream of the process on that device, a torch or RCCL side stream included
        int cur = 0;
        if (hipGetDevice(&cur) != hipSuccess) return false;
        if (cur != device && hipSetDevice(device) != hipSuccess) return false;
        const hipError_t e = hipDeviceSynchronize();
        if (cur != device) (void)hipSetDevice(cur);
        return e == hipSuccess;
    }
};
wdgs::AllocCache<HipBackend> g_alloc_cache;
size_t g_cache_limit = 0;
std::mutex g_cache_limit_mutex;
bool alloc_cache_enabled() {
    static const bool on = !(std::getenv("WDGS_ALLOC_CACHE") && std::getenv("WDGS_ALLOC_CACHE")[0] == '0');
    return on;
}
}  // namespace

int wdgs_alloc(void** p, size_t bytes, bool zero, hipStream_t stream) {
    *p = nullptr;
    if (bytes == 0) bytes = 16;
    if (!alloc_cache_enabled()) {
        WDGS_CHECK_HIP(hipMalloc(p, bytes));
    } else {
        int device = 0;
        WDGS_CHECK_HIP(hipGetDevice(&device));
        // (an allocation while `stream` records -- relaxed capture allows hipMalloc -- cannot synchronise the device: it only takes blocks that need no wait)
        hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
        const bool recording = stream && hipStreamIsCapturing(stream, &capture) == hipSuccess && capture != hipStreamCaptureStatusNone;
        *p = g_alloc_cache.alloc(device, bytes, !recording);
        WDGS_REQUIRE(*p, WDGS_E_HIP, "device allocation of %zu bytes failed (device %d)", bytes, device);
    }
    if (zero) WDGS_CHECK_HIP(hipMemsetAsync(*p, 0, bytes, stream));
    return WDGS_OK;
}

void wdgs_free(void* p) {
    if (!p) return;
    if (alloc_cache_enabled()) {
        size_t limit;
        {
            std::lock_guard<std::mutex> lock(g_cache_limit_mutex);
            if (g_cache_limit == 0) {
                size_t free_b = 0, total_b = 0;
                g_cache_limit = (hipMemGetInfo(&free_b, &total_b) == hipSuccess && total_b) ? total_b / 4 : ((size_t)8 << 30);
            }
            limit = g_cache_limit;
        }
        if (g_alloc_cache.free(p, limit)) return;
    }
    (void)hipFree(p);
}

// ---- the op structs.  Every block of device memory an op owns is a DevMem member (devmem.h), so `delete op` frees what the op holds and a create
// function that fails half way has nothing to undo; the destroy functions below keep only what is specific to their op (and the wait for the device,
// which comes before the delete).
struct wdgs_buffer {
    DevMem<char> mem;   // count() is the size in bytes
};

struct wdgs_prefix_scanner {
    wdgs_device* dev = nullptr;
    u32 max_elements = 0, count = 0;
    DevMem<u32> input, output;
    ScanScratch scratch;
};

struct SorterDelete { void operator()(wdgs_sorter* s) const { wdgs_sorter_destroy(s); } };

struct wdgs_tiled_forward {
    wdgs_device* dev = nullptr;
    wdgs_tiled_forward_config cfg = {};
    RenderSettings settings = {};
    TileInfo tile_info = {};
    DevMem<u32> stats;   // {total_tile_entries, visible_gaussians, overflow (0 or requested total), pad} + 64 visible-count shards + the frame number (FRAME_WORD)
    // u32[tiles]: a tile whose entry equals the frame number holds a Splat with a NaN or an infinity among its fp16 fields (project.hip stamps,
    // scan.hip advances the number, raster.hip takes such tiles in the oracle's own forms)
    DevMem<u32> nf_stamp;
    // Long tile lists (longlist.h): tables, scratch and the per-tile marks; `long_lists.hdr == nullptr`: switched off.  Built by this pass's sort, used by
    // the rasterizer that composites with this pass's range table and by a backward pass that is handed that table (found through dev->range_tables).
    // long_lists is what the kernels are handed: pointers into long_base (one allocation, the tables carved out of it), to long_flags and to nf_stamp.
    LongWork long_lists = {};
    DevMem<char> long_base;
    DevMem<u32> long_flags;   // u32[tiles]
    u32* host_stats = nullptr;  // pinned, device-visible copy of stats[0..3] written by update_stats: the per-step overflow check reads host memory
    DevMem<u32> splats;
    DevMem<u32> depths;
    DevMem<u32> block_counts;  // u32[ceil(N/256)]: tile entries per project_count workgroup, scanned in place into workgroup offsets
    // u32[256][ceil(N/256)] + u32[256]: tile entries per workgroup and tile COLUMN (project_count), scanned per column into the workgroup's
    // offset inside the column, and the column totals -- the digit counts of the sort's first pass, which emit_scatter performs (project.hip)
    DevMem<u32> column_counts;
    DevMem<u32> column_totals;
    const u32* dc_source = nullptr;  // nullable: the optimizer's compact SH-DC words (wdgs_tiled_forward_set_dc_source), read by project_count in place of the rows' first 6 bytes
    // Gaussians the per-Gaussian buffers above and the scanner hold (>= cfg.num_points: wdgs_tiled_forward_resize); 0 while they are not all there
    u32 points_capacity = 0;
    std::unique_ptr<wdgs_prefix_scanner> scanner;  // input = tile counts, output = per-Gaussian offsets
    std::unique_ptr<wdgs_sorter, SorterDelete> sorter;
    // Per-tile range table u32[tiles + 1].  The sort of tile-structured keys needs it half way (sort.hip, sort_segmented), so the
    // forward pass builds it and the rasterizer -- which owns K12-K13 in the reference (tiled-rasterizer.ts:213-230) -- takes it over
    // instead of searching the keys a second time.  Not valid after encode(skip_sort) or under compat_caps (plain 4-pass sort).
    DevMem<u32> ranges;
    bool ranges_valid = false;
    bool encoded = false;
    bool projected = false;          // K1 of the current frame ran through wdgs_tiled_forward_project_views
    bool projected_columns = false;  // ... and counted per tile column
    ~wdgs_tiled_forward() { if (host_stats) (void)hipHostFree(host_stats); }
};

constexpr u32 FRAME_WORD = 4u + 64u;   // index of the frame number in wdgs_tiled_forward::stats
constexpr size_t FORWARD_STATS_BYTES = 16 + 64 * 4 + 16;

struct wdgs_tiled_rasterizer {
    wdgs_device* dev = nullptr;
    wdgs_tiled_forward* fwd = nullptr;
    u32 compat_caps = 0;
    u32 width = 0, height = 0;   // size of the three images below; 0 x 0 while they are not all there
    DevMem<u32> ranges;          // own table, u32[tiles + 1] (used when the forward pass did not build one)
    u32* ranges_used = nullptr;  // the table the last encode composited with: own or the forward pass's
    DevMem<u32> rgba8;
    DevMem<float> alpha;
    DevMem<u32> n_contrib;
    bool encoded = false;
    // depth images (depth.hip), f32[W*H] each, in the order of the WDGS_DEPTH_* bits: allocated per kind at its first encode_depth
    DevMem<float> depth[3];
    u32 depth_width = 0, depth_height = 0;   // the size they were allocated for
    u32 depth_encoded = 0;                   // the kinds the last encode_depth wrote
    // normals (normal.hip): one packed word per Gaussian and the composited image { N.xyz, A }, allocated at the first encode_normal
    DevMem<u32> normals;
    u32 normals_points = 0;                  // the point count the words were allocated for
    DevMem<float4> normal_image;
    u32 normal_width = 0, normal_height = 0; // the size it was allocated for
    bool normal_encoded = false;
};

struct wdgs_tiled_backward {
    wdgs_device* dev = nullptr;
    wdgs_tiled_backward_config cfg = {};
    RenderSettings settings = {};
    DevMem<int> acc;     // i32[capacity*12], followed by the state word below (and 12 bytes of padding)
    // device word behind the accumulators: 0 = all rows are zero (a consuming K17 left them so), 1 = they hold sums
    u32* acc_dirty() const { return acc ? reinterpret_cast<u32*>(acc.get() + (acc.count() - 4)) : nullptr; }
    DevMem<u32> gradients;      // GaussianGradient[N]
    bool gradient_output = true;  // the fused K17 + Adam step also writes the packed gradient (wdgs_tiled_backward_set_gradient_output; default on)
    DevMem<float4> loss_image;  // rgba32f[W*H]
    u32 dssim_mode = 0;  // WDGS_DSSIM_*: the loss kernel an encode launches (wdgs_tiled_backward_set_dssim_mode)
    DevMem<u32> metric_counts;  // u32[N]
    u32* metric_counts_into = nullptr;  // nullable: computeMetricCounts adds into THIS array instead (wdgs_tiled_backward_set_metric_counts_target)
    DevMem<u32> metric_err;     // u32[W*H]
    DevMem<u32> metric_flags;   // u32[W*H]: its count() is the pixels all three images hold (backward_alloc_images)
    DevMem<u32> metric_minmax;  // u32[2] + scratch
    u32 points_capacity = 0;  // Gaussians acc / gradients / metric_counts hold (>= cfg.num_points: wdgs_tiled_backward_resize); 0 while they are not all there
};

struct wdgs_optimizer {
    wdgs_device* dev = nullptr;
    u32 num_points = 0;
    wdgs_adam_hyperparameters params = {0.00016f, 0.0025f, 0.05f, 0.005f, 0.001f, 0.9f, 0.999f, 1e-8f};  // adam-config.ts:12-21
    wdgs_optimizer_state state = {};   // the view of the six arrays that kernels and wdgs_optimizer_get_state are handed
    // ... and their owners, in the order of state's fields, when the optimizer owns them: allocated here or adopted from the host (owns_state at
    // creation), emptied without freeing by wdgs_optimizer_release_state
    DevMem<char> owned[6];
    bool owns_state() const { return bool(owned[0]); }
    u32 iteration = 0;
    DevMem<float4> dc;  // compact training copy, float4[7][max(N, 1)] planes: position, log-scale and SH-DC {param, m, v} (adam.h; optimizer.hip "HBM layout note"); always owned
    static u32 cs_pitch(u32 n) { return (std::max(n, 1u) + 15u) & ~15u; }  // planes start on 256-byte boundaries
    CsView cs() const { return CsView{dc.get(), cs_pitch(num_points)}; }
    bool dc_dirty = false;    // it is ahead of state.opt_pos / opt_scale / param_sh / state_sh
    const u32* guard = nullptr;  // device word: non-zero at execution time turns step / step_f32 into a no-op (wdgs_optimizer_set_guard)
    // Deferred SH writes (wdgs_optimizer_set_deferred_sh): the steps write the trained DC halves to dc_words (u32[N][2]) instead of the
    // 96-byte rows; sh_stale says the rows are behind until wdgs_optimizer_flush_sh.
    DevMem<u32> dc_words;
    bool deferred_sh = false;
    bool sh_stale = false;
};

// Brings the reference-layout arrays (position, log-scale, SH) up to date with the compact training copy (no-op when nothing was trained since).
static int optimizer_flush_dc(wdgs_optimizer* op) {
    if (!op->dc_dirty) return WDGS_OK;
    WDGS_TRY(launch_cs_flush(op->dev, op->num_points, op->cs(), op->state));
    op->dc_dirty = false;
    return WDGS_OK;
}

extern "C" {

const char* wdgs_last_error(void) { return g_last_error; }
int wdgs_abi_version(void) { return 1; }

// ---------------------------------------------------------------- device
int wdgs_device_create(int ordinal, void* external_stream, wdgs_device** out) {
    WDGS_REQUIRE(out, WDGS_E_INVALID, "wdgs_device_create: out is null");
    int count = 0;
    WDGS_CHECK_HIP(hipGetDeviceCount(&count));
    WDGS_REQUIRE(ordinal >= 0 && ordinal < count, WDGS_E_INVALID, "wdgs_device_create: ordinal %d out of range (%d devices)", ordinal, count);
    WDGS_CHECK_HIP(hipSetDevice(ordinal));
    wdgs_device* d = new wdgs_device();
    d->ordinal = ordinal;
    if (external_stream) {
        d->stream = (hipStream_t)external_stream;
        d->own_stream = false;
    } else {
        hipError_t e = hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking);
        if (e != hipSuccess) { delete d; wdgs_set_error("hipStreamCreate failed: %s", hipGetErrorString(e)); return WDGS_E_HIP; }
        d->own_stream = true;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, ordinal) == hipSuccess) d->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    d->lanes[0] = d->stream;
    if (hipHostMalloc((void**)&d->host_guard, 16, hipHostMallocDefault) != hipSuccess) {
        wdgs_set_error("hipHostMalloc(16) failed");
        if (d->own_stream) (void)hipStreamDestroy(d->stream);
        delete d;
        return WDGS_E_HIP;
    }
    std::memset(d->host_guard, 0, 16);
    { std::lock_guard<std::mutex> lock(g_live_mutex); g_live_devices.insert(d); }
    *out = d;
    return WDGS_OK;
}

// ---- lanes: in-order streams of one device, ordered against each other only where the host says so ----
int wdgs_device_select_lane(wdgs_device* d, int lane) {
    WDGS_REQUIRE(d, WDGS_E_INVALID, "wdgs_device_select_lane: null device");
    WDGS_REQUIRE(lane >= 0 && lane < WDGS_MAX_LANES, WDGS_E_INVALID, "wdgs_device_select_lane: lane %d (0..%d)", lane, WDGS_MAX_LANES - 1);
    WDGS_REQUIRE(!d->capturing, WDGS_E_STATE, "wdgs_device_select_lane while recording a command buffer");
    WDGS_CHECK_HIP(hipSetDevice(d->ordinal));
    if (!d->lanes[lane]) WDGS_CHECK_HIP(hipStreamCreateWithFlags(&d->lanes[lane], hipStreamNonBlocking));
    d->stream = d->lanes[lane];
    d->lane = lane;
    return WDGS_OK;
}

int wdgs_device_lane_order(wdgs_device* d, int waiter, int signal) {
    WDGS_REQUIRE(d, WDGS_E_INVALID, "wdgs_device_lane_order: null device");
    WDGS_REQUIRE(waiter >= 0 && waiter < WDGS_MAX_LANES && signal >= 0 && signal < WDGS_MAX_LANES, WDGS_E_INVALID, "wdgs_device_lane_order: lanes %d, %d (0..%d)", waiter,
                 signal, WDGS_MAX_LANES - 1);
    WDGS_REQUIRE(!d->capturing, WDGS_E_STATE, "wdgs_device_lane_order while recording a command buffer");
    if (waiter == signal || !d->lanes[signal]) return WDGS_OK;  // a lane is in order with itself; a lane never used has nothing pending
    WDGS_CHECK_HIP(hipSetDevice(d->ordinal));
    if (!d->lanes[waiter]) WDGS_CHECK_HIP(hipStreamCreateWithFlags(&d->lanes[waiter], hipStreamNonBlocking));
    // one event per signalling lane: a wait refers to the record that precedes it, so re-recording the event later is safe
    if (!d->lane_events[signal]) WDGS_CHECK_HIP(hipEventCreateWithFlags(&d->lane_events[signal], hipEventDisableTiming));
    WDGS_CHECK_HIP(hipEventRecord(d->lane_events[signal], d->lanes[signal]));
    WDGS_CHECK_HIP(hipStreamWaitEvent(d->lanes[waiter], d->lane_events[signal], 0));
    return WDGS_OK;
}

// A position on a lane, kept in one of WDGS_MAX_BATCH_VIEWS numbered marks, that other lanes can be made to wait for LATER (lane_order
// records and waits in one call): a batched step projects its view groups one after the other on one lane and lets each view wait only
// for its own group's projection.
int wdgs_device_lane_mark(wdgs_device* d, int lane, int mark) {
    WDGS_REQUIRE(d && lane >= 0 && lane < WDGS_MAX_LANES && mark >= 0 && mark < WDGS_MAX_BATCH_VIEWS, WDGS_E_INVALID, "wdgs_device_lane_mark: lane %d, mark %d", lane, mark);
    WDGS_REQUIRE(!d->capturing, WDGS_E_STATE, "wdgs_device_lane_mark while recording a command buffer");
    WDGS_CHECK_HIP(hipSetDevice(d->ordinal));
    if (!d->lanes[lane]) WDGS_CHECK_HIP(hipStreamCreateWithFlags(&d->lanes[lane], hipStreamNonBlocking));
    if (!d->lane_marks[mark]) WDGS_CHECK_HIP(hipEventCreateWithFlags(&d->lane_marks[mark], hipEventDisableTiming));
    WDGS_CHECK_HIP(hipEventRecord(d->lane_marks[mark], d->lanes[lane]));
    return WDGS_OK;
}
int wdgs_device_lane_wait_mark(wdgs_device* d, int lane, int mark) {
    WDGS_REQUIRE(d && lane >= 0 && lane < WDGS_MAX_LANES && mark >= 0 && mark < WDGS_MAX_BATCH_VIEWS, WDGS_E_INVALID, "wdgs_device_lane_wait_mark: lane %d, mark %d", lane, mark);
    WDGS_REQUIRE(!d->capturing, WDGS_E_STATE, "wdgs_device_lane_wait_mark while recording a command buffer");
    WDGS_REQUIRE(d->lane_marks[mark], WDGS_E_STATE, "wdgs_device_lane_wait_mark: mark %d was never set", mark);
    WDGS_CHECK_HIP(hipSetDevice(d->ordinal));
    if (!d->lanes[lane]) WDGS_CHECK_HIP(hipStreamCreateWithFlags(&d->lanes[lane], hipStreamNonBlocking));
    WDGS_CHECK_HIP(hipStreamWaitEvent(d->lanes[lane], d->lane_marks[mark], 0));
    return WDGS_OK;
}

// Folds the finished event pairs into the per-kernel totals.  Pairs whose kernels have not finished yet (a wait for an earlier ticket,
// a query between steps) stay pending: events of one queue complete in order, so the scan stops at the first unfinished pair.
static int collect_profile(wdgs_device* d) {
    size_t done = 0;
    for (auto& p : d->pending) {
        float ms = 0.f;
        const hipError_t e = hipEventElapsedTime(&ms, p.a, p.b);
        if (e == hipErrorNotReady) { (void)hipGetLastError(); break; }
        if (e == hipSuccess) {
            auto& t = d->totals[p.name];
            t.launches += 1;
            t.ms += ms;
        }
        d->event_pool.push_back(p.a);
        d->event_pool.push_back(p.b);
        done++;
    }
    d->pending.erase(d->pending.begin(), d->pending.begin() + (long)done);
    return WDGS_OK;
}

// Device-side conditions that are reported at the next host wait: a truncated tile-entry list (per forward pass, sticky since its last
// check) and a guarded optimizer step that skipped itself (sticky; set when the guard word of a batched / data-parallel step was
// non-zero -- on this rank or, after the exchange summed it, on any other).  Reading consumes them.
static int deferred_checks(wdgs_device* d) {
    // The words are consumed with an atomic exchange: a wait for step k's ticket runs while step k+1 is in flight (pipeline depth 2),
    // and a read followed by a plain store of 0 would lose a note the device writes between the two.  The device writes
    // whole aligned words into pinned host memory; the exchange either sees the note (and reports it now) or leaves it for the next check.
    const u32 skipped = __atomic_exchange_n(d->host_guard, 0u, __ATOMIC_ACQ_REL);
    // every pass's word is consumed; the report names every pass that overflowed (up to four), so that a host whose passes share the device with
    // another owner's -- a Trainer beside a Viewer -- can tell its own
    char report[384];
    size_t at = 0;
    u32 found = 0u;
    for (wdgs_tiled_forward* f : d->forwards) {
        if (!f->encoded) continue;
        // written by update_stats before the stream drained (no device round trip here); sticky across the encodes since the last
        // check: the exchange consumes it
        const u32 v = __atomic_exchange_n(f->host_stats + 2, 0u, __ATOMIC_ACQ_REL);
        if (v != 0u && found < 4u && at < sizeof(report)) {
            const int w = std::snprintf(report + at, sizeof(report) - at, "%s%u entries needed, max_tile_entries = %u (forward pass %p)", found ? "; " : "", v,
                                        f->tile_info.max_tile_entries, (void*)f);
            if (w > 0) at += (size_t)w;
            found++;
        }
    }
    WDGS_REQUIRE(found == 0u, WDGS_E_CAPACITY, "tile entries overflow: %s (raise wdgs_tiled_forward_config.max_tile_entries)", report);
    WDGS_REQUIRE(skipped == 0u, WDGS_E_CAPACITY, "an optimizer step was skipped on every rank: tile entries overflowed on another rank (its own error names the size)");
    return WDGS_OK;
}

int wdgs_device_synchronize(wdgs_device* d) {
    WDGS_REQUIRE(d, WDGS_E_INVALID, "wdgs_device_synchronize: null device");
    WDGS_REQUIRE(!d->capturing, WDGS_E_STATE, "wdgs_device_synchronize while recording a command buffer");
    WDGS_CHECK_HIP(hipSetDevice(d->ordinal));
    WDGS_CHECK_HIP(wdgs_sync_lanes(d));
    collect_profile(d);
    return deferred_checks(d);
}

int wdgs_queue_mark(wdgs_device* d, uint64_t* ticket) {
    WDGS_REQUIRE(d && ticket, WDGS_E_INVALID, "wdgs_queue_mark: null argument");
    WDGS_REQUIRE(!d->capturing, WDGS_E_STATE, "wdgs_queue_mark while recording a command buffer");
    WDGS_CHECK_HIP(hipSetDevice(d->ordinal));
    const uint64_t t = d->ticket_next;
    hipEvent_t& e = d->ticket_events[t % WDGS_TICKET_RING];
    if (!e) WDGS_CHECK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    WDGS_CHECK_HIP(hipEventRecord(e, d->stream));
    d->ticket_next = t + 1;
    *ticket = t;
    return WDGS_OK;
}

int wdgs_queue_wait(wdgs_device* d, uint64_t ticket) {
    WDGS_REQUIRE(d, WDGS_E_INVALID, "wdgs_queue_wait: null device");
    WDGS_REQUIRE(ticket != 0 && ticket < d->ticket_next, WDGS_E_INVALID, "wdgs_queue_wait: ticket %llu was never issued", (unsigned long long)ticket);
    WDGS_REQUIRE(!d->capturing, WDGS_E_STATE, "wdgs_queue_wait while recording a command buffer");
    // (a ticket older than the ring waits on the mark that took its slot: later in the same queue, so the wait still holds)
    WDGS_CHECK_HIP(hipEventSynchronize(d->ticket_events[ticket % WDGS_TICKET_RING]));
    if (!d->pending.empty()) collect_profile(d);
    return deferred_checks(d);
}

int wdgs_device_memory_info(wdgs_device* d, size_t* free_bytes, size_t* total_bytes, size_t* cached_bytes) {
    WDGS_REQUIRE(d, WDGS_E_INVALID, "wdgs_device_memory_info: null device");
    size_t f = 0, t = 0;
    WDGS_CHECK_HIP(hipSetDevice(d->ordinal));
    WDGS_CHECK_HIP(hipMemGetInfo(&f, &t));
    if (free_bytes) *free_bytes = f;
    if (total_bytes) *total_bytes = t;
    if (cached_bytes) *cached_bytes = g_alloc_cache.held(d->ordinal);
    return WDGS_OK;
}
static void reap_command_buffers(wdgs_device* d, size_t at_most);   // (defined with the command buffers, below)
int wdgs_device_destroy(wdgs_device* d) {
    if (!d) return WDGS_OK;
    {
        std::lock_guard<std::mutex> lock(g_live_mutex);
        if (!g_live_devices.erase(d)) return WDGS_OK;  // already destroyed (or never ours): idempotent
    }
    (void)hipSetDevice(d->ordinal);
    if (d->capturing) {  // an abandoned recording: end it so the stream is usable by its owner again
        hipGraph_t g = nullptr;
        (void)hipStreamEndCapture(d->stream, &g);
        if (g) (void)hipGraphDestroy(g);
        d->capturing = false;
    }
    (void)wdgs_sync_lanes(d);
    collect_profile(d);
    reap_command_buffers(d, (size_t)-1);
    g_alloc_cache.release(d->ordinal);
    for (hipEvent_t e : d->event_pool) (void)hipEventDestroy(e);
    for (hipEvent_t e : d->lane_events) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : d->lane_marks) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : d->ticket_events) if (e) (void)hipEventDestroy(e);
    if (d->host_guard) (void)hipHostFree(d->host_guard);
    if (d->ssim_partials) (void)hipFree(d->ssim_partials);
    for (int l = 1; l < WDGS_MAX_LANES; l++)
        if (d->lanes[l]) (void)hipStreamDestroy(d->lanes[l]);
    if (d->own_stream) (void)hipStreamDestroy(d->lanes[0]);
    delete d;
    return WDGS_OK;
}

int wdgs_device_set_profiling(wdgs_device* d, int enabled) {
    WDGS_REQUIRE(d, WDGS_E_INVALID, "null device");
    d->profiling = enabled != 0;
    return WDGS_OK;
}

int wdgs_device_get_kernel_times(wdgs_device* d, wdgs_kernel_time* out, uint32_t cap, uint32_t* count) {
    WDGS_REQUIRE(d && count, WDGS_E_INVALID, "null argument");
    if (!d->pending.empty() && !d->capturing) collect_profile(d);  // (whatever has finished by now; a synchronize before the call makes that everything)
    u32 i = 0;
    for (auto& kv : d->totals) {
        if (out && i < cap) {
            std::memset(&out[i], 0, sizeof(out[i]));
            std::strncpy(out[i].name, kv.first.c_str(), sizeof(out[i].name) - 1);
            out[i].launches = kv.second.launches;
            out[i].total_ms = kv.second.ms;
        }
        i++;
    }
    *count = i;
    return WDGS_OK;
}

int wdgs_device_reset_kernel_times(wdgs_device* d) {
    WDGS_REQUIRE(d, WDGS_E_INVALID, "null device");
    d->totals.clear();
    return WDGS_OK;
}

// ---------------------------------------------------------------- recorded command buffers
static bool forward_holds_projection(const wdgs_tiled_forward* f);
static void forward_consume_projection(wdgs_tiled_forward* f);
// `consumes`: the forward passes whose projection (wdgs_tiled_forward_project_views) a replay of this recording uses up -- its scan works in
// place on K1's workgroup sums.  The validity flag of a pass is a HOST fact checked when an encode is made; a replay makes no encode call, so
// the command buffer carries the check to wdgs_queue_submit.  Without it a recording that starts at the scan could be replayed on a pass whose
// projection another encode had already consumed: offsets scanned twice, a tile-entry count far beyond the entries really written, stale keys
// with a zero tile field among them, and sort_scatter's atomicMin(&ranges[(key >> 16) - 1]) landing 16 GB past the table -- the device fault
// behind the abort of gpurun_out/r04o_tests.log.
struct wdgs_command_buffer_impl { hipGraph_t graph; hipGraphExec_t exec; std::vector<wdgs_tiled_forward*> consumes; wdgs_device* dev; };
static void command_buffer_release(wdgs_command_buffer_impl* c) {
    (void)hipGraphExecDestroy(c->exec);
    (void)hipGraphDestroy(c->graph);
    delete c;
}
static void reap_command_buffers(wdgs_device* d, size_t at_most) {
    while (at_most-- && !d->dead_command_buffers.empty()) {
        command_buffer_release(static_cast<wdgs_command_buffer_impl*>(d->dead_command_buffers.back()));
        d->dead_command_buffers.pop_back();
    }
}

int wdgs_encoder_begin(wdgs_device* d) {
    WDGS_REQUIRE(d, WDGS_E_INVALID, "null device");
    WDGS_REQUIRE(!d->capturing, WDGS_E_STATE, "wdgs_encoder_begin: a recording is already open on this device");
    WDGS_CHECK_HIP(hipStreamBeginCapture(d->stream, hipStreamCaptureModeRelaxed));
    d->capturing = true;
    d->capture_consumes.clear();
    return WDGS_OK;
}
int wdgs_encoder_finish(wdgs_device* d, wdgs_command_buffer** out) {
    WDGS_REQUIRE(d && out, WDGS_E_INVALID, "null argument");
    WDGS_REQUIRE(d->capturing, WDGS_E_STATE, "wdgs_encoder_finish without wdgs_encoder_begin");
    d->capturing = false;
    hipGraph_t graph = nullptr;
    WDGS_CHECK_HIP(hipStreamEndCapture(d->stream, &graph));
    hipGraphExec_t exec = nullptr;
    hipError_t e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    if (e != hipSuccess) { (void)hipGraphDestroy(graph); d->capture_consumes.clear(); wdgs_set_error("hipGraphInstantiate failed: %s", hipGetErrorString(e)); return WDGS_E_HIP; }
    auto* c = new wdgs_command_buffer_impl{graph, exec, std::move(d->capture_consumes), d};
    d->capture_consumes.clear();
    *out = reinterpret_cast<wdgs_command_buffer*>(c);
    return WDGS_OK;
}
int wdgs_encoder_abort(wdgs_device* d) {
    WDGS_REQUIRE(d, WDGS_E_INVALID, "null device");
    if (!d->capturing) return WDGS_OK;  // nothing open: harmless, so error paths may call it unconditionally
    d->capturing = false;
    d->capture_consumes.clear();
    hipGraph_t graph = nullptr;
    const hipError_t e = hipStreamEndCapture(d->stream, &graph);  // an invalidated capture reports an error here and yields no graph
    if (graph) (void)hipGraphDestroy(graph);
    (void)hipGetLastError();  // the failed encode's sticky error, if any, belongs to the aborted recording
    (void)e;
    return WDGS_OK;
}
int wdgs_queue_submit(wdgs_device* d, wdgs_command_buffer* cmd) {
    WDGS_REQUIRE(d && cmd, WDGS_E_INVALID, "null argument");
    WDGS_REQUIRE(!d->capturing, WDGS_E_STATE, "wdgs_queue_submit while recording");
    auto* c = reinterpret_cast<wdgs_command_buffer_impl*>(cmd);
    // a recording that contains wdgs_tiled_forward_encode_projected uses up the projection of its pass on EVERY replay: all must be there
    // (checked before anything is consumed, so a refused submit changes nothing)
    for (wdgs_tiled_forward* f : c->consumes) {
        WDGS_REQUIRE(std::find(d->forwards.begin(), d->forwards.end(), f) != d->forwards.end(), WDGS_E_STATE,
                     "wdgs_queue_submit: the command buffer was recorded against a forward pass that has been destroyed");
        WDGS_REQUIRE(forward_holds_projection(f), WDGS_E_STATE,
                     "wdgs_queue_submit: the command buffer starts at the scan of a projected forward pass (wdgs_tiled_forward_encode_projected), but the pass holds no "
                     "projection: run wdgs_tiled_forward_project_views before every submit, and no other encode of the pass in between");
    }
    WDGS_CHECK_HIP(hipGraphLaunch(c->exec, d->stream));
    for (wdgs_tiled_forward* f : c->consumes) forward_consume_projection(f);   // (only a replay that was really enqueued uses the projections up)
    reap_command_buffers(d, 1);   // (behind the launch: the device is busy with it while the host pays)
    return WDGS_OK;
}
namespace {
struct DoneThunk { wdgs_done_callback fn; void* user; };
void done_trampoline(void* p) {
    DoneThunk* t = static_cast<DoneThunk*>(p);
    t->fn(t->user);
    delete t;
}
}  // namespace
int wdgs_queue_on_done(wdgs_device* d, wdgs_done_callback fn, void* user) {
    WDGS_REQUIRE(d && fn, WDGS_E_INVALID, "wdgs_queue_on_done: null argument");
    WDGS_REQUIRE(!d->capturing, WDGS_E_STATE, "wdgs_queue_on_done while recording a command buffer");
    DoneThunk* t = new DoneThunk{fn, user};
    hipError_t e = hipLaunchHostFunc(d->stream, done_trampoline, t);
    if (e != hipSuccess) { delete t; wdgs_set_error("hipLaunchHostFunc failed: %s", hipGetErrorString(e)); return WDGS_E_HIP; }
    return WDGS_OK;
}
int wdgs_command_buffer_destroy(wdgs_command_buffer* cmd) {
    if (!cmd) return WDGS_OK;
    auto* c = reinterpret_cast<wdgs_command_buffer_impl*>(cmd);
    // WDGS_LAZY_GRAPH_DESTROY=0: destroy here and now
    static const bool lazy = !(std::getenv("WDGS_LAZY_GRAPH_DESTROY") && std::getenv("WDGS_LAZY_GRAPH_DESTROY")[0] == '0');
    if (lazy && wdgs_device_alive(c->dev)) {
        c->dev->dead_command_buffers.push_back(c);
        if (c->dev->dead_command_buffers.size() > 64u) reap_command_buffers(c->dev, 32u);   // (a host that never submits again must not pile them up)
    } else command_buffer_release(c);
    return WDGS_OK;
}

int wdgs_copy_to_host(wdgs_device* d, void* dst, const void* src, size_t bytes) {
    WDGS_REQUIRE(d && (bytes == 0 || (dst && src)), WDGS_E_INVALID, "wdgs_copy_to_host: null argument");
    WDGS_REQUIRE(!d->capturing, WDGS_E_STATE, "wdgs_copy_to_host while recording a command buffer");
    if (bytes == 0) return WDGS_OK;
    WDGS_CHECK_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, d->stream));
    WDGS_CHECK_HIP(wdgs_sync_lanes(d));
    return WDGS_OK;
}

int wdgs_copy_to_device(wdgs_device* d, void* dst, const void* src, size_t bytes) {
    WDGS_REQUIRE(d && (bytes == 0 || (dst && src)), WDGS_E_INVALID, "wdgs_copy_to_device: null argument");
    // a recording would bake the (pageable, soon reused) host pointer into the graph: uploads belong before wdgs_encoder_begin
    WDGS_REQUIRE(!d->capturing, WDGS_E_STATE, "wdgs_copy_to_device while recording a command buffer");
    if (bytes == 0) return WDGS_OK;
    // pageable source: hipMemcpyAsync stages the copy before returning, so `src` may be reused immediately
    WDGS_CHECK_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, d->stream));
    return WDGS_OK;
}

int wdgs_memset(wdgs_device* d, void* dst, int value, size_t bytes) {
    WDGS_REQUIRE(d && (bytes == 0 || dst), WDGS_E_INVALID, "wdgs_memset: null argument");
    if (bytes == 0) return WDGS_OK;
    // allowed inside a recording: it becomes a memset node of the command buffer (encoder.clearBuffer is recorded in the reference too)
    WDGS_CHECK_HIP(hipMemsetAsync(dst, value, bytes, d->stream));
    return WDGS_OK;
}

int wdgs_copy_buffer_to_buffer(wdgs_device* d, void* dst, const void* src, size_t bytes) {
    WDGS_REQUIRE(d && (bytes == 0 || (dst && src)), WDGS_E_INVALID, "wdgs_copy_buffer_to_buffer: null argument");
    if (bytes == 0) return WDGS_OK;
    // device to device, stream-ordered; inside a recording it becomes a copy node (encoder.copyBufferToBuffer is recorded in the reference too)
    WDGS_CHECK_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, d->stream));
    return WDGS_OK;
}

// ---------------------------------------------------------------- buffers
int wdgs_buffer_create(wdgs_device* d, size_t bytes, wdgs_buffer** out) {
    WDGS_REQUIRE(d && out, WDGS_E_INVALID, "wdgs_buffer_create: null argument");
    auto b = std::make_unique<wdgs_buffer>();
    WDGS_TRY(b->mem.alloc(bytes, true, d->stream));
    *out = b.release();
    return WDGS_OK;
}
int wdgs_buffer_destroy(wdgs_buffer* b) {
    delete b;
    return WDGS_OK;
}
void* wdgs_buffer_ptr(const wdgs_buffer* b) { return b ? b->mem.get() : nullptr; }
size_t wdgs_buffer_size(const wdgs_buffer* b) { return b ? b->mem.count() : 0; }
int wdgs_buffer_write(wdgs_device* d, wdgs_buffer* b, size_t off, const void* src, size_t bytes) {
    WDGS_REQUIRE(d && b, WDGS_E_INVALID, "wdgs_buffer_write: null argument");
    WDGS_REQUIRE(off + bytes <= b->mem.count(), WDGS_E_INVALID, "wdgs_buffer_write: range [%zu, %zu) exceeds buffer size %zu", off, off + bytes, b->mem.count());
    return wdgs_copy_to_device(d, b->mem.get() + off, src, bytes);
}
int wdgs_buffer_read(wdgs_device* d, const wdgs_buffer* b, size_t off, void* dst, size_t bytes) {
    WDGS_REQUIRE(d && b, WDGS_E_INVALID, "wdgs_buffer_read: null argument");
    WDGS_REQUIRE(off + bytes <= b->mem.count(), WDGS_E_INVALID, "wdgs_buffer_read: range [%zu, %zu) exceeds buffer size %zu", off, off + bytes, b->mem.count());
    return wdgs_copy_to_host(d, dst, b->mem.get() + off, bytes);
}
int wdgs_buffer_read_async(wdgs_device* d, const wdgs_buffer* b, size_t off, void* dst, size_t bytes) {
    WDGS_REQUIRE(d && b && (bytes == 0 || dst), WDGS_E_INVALID, "wdgs_buffer_read_async: null argument");
    WDGS_REQUIRE(off + bytes <= b->mem.count(), WDGS_E_INVALID, "wdgs_buffer_read_async: range [%zu, %zu) exceeds buffer size %zu", off, off + bytes, b->mem.count());
    WDGS_REQUIRE(!d->capturing, WDGS_E_STATE, "wdgs_buffer_read_async while recording a command buffer");
    if (bytes == 0) return WDGS_OK;
    WDGS_CHECK_HIP(hipMemcpyAsync(dst, b->mem.get() + off, bytes, hipMemcpyDeviceToHost, d->stream));
    return WDGS_OK;
}
int wdgs_host_alloc(size_t bytes, void** out) {
    WDGS_REQUIRE(out, WDGS_E_INVALID, "wdgs_host_alloc: null argument");
    WDGS_CHECK_HIP(hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault));
    return WDGS_OK;
}
int wdgs_host_free(void* p) {
    if (p) WDGS_CHECK_HIP(hipHostFree(p));
    return WDGS_OK;
}

// ---------------------------------------------------------------- prefix scanner
int wdgs_prefix_scanner_create(wdgs_device* d, uint32_t max_elements, wdgs_prefix_scanner** out) {
    WDGS_REQUIRE(d && out, WDGS_E_INVALID, "wdgs_prefix_scanner_create: null argument");
    auto s = std::make_unique<wdgs_prefix_scanner>();
    s->dev = d;
    s->max_elements = max_elements > 0 ? max_elements : 1;
    s->count = s->max_elements;
    WDGS_TRY(s->input.alloc(s->max_elements, true, d->stream));
    WDGS_TRY(s->output.alloc(s->max_elements, true, d->stream));
    WDGS_TRY(scan_scratch_create(&s->scratch, s->max_elements));
    *out = s.release();
    return WDGS_OK;
}
int wdgs_prefix_scanner_destroy(wdgs_prefix_scanner* s) {
    delete s;
    return WDGS_OK;
}
void* wdgs_prefix_scanner_input(wdgs_prefix_scanner* s) { return s ? s->input.get() : nullptr; }
void* wdgs_prefix_scanner_output(wdgs_prefix_scanner* s) { return s ? s->output.get() : nullptr; }
int wdgs_prefix_scanner_set_count(wdgs_prefix_scanner* s, uint32_t count) {
    WDGS_REQUIRE(s, WDGS_E_INVALID, "null scanner");
    WDGS_REQUIRE(count <= s->max_elements, WDGS_E_CAPACITY, "scan count %u exceeds max_elements %u", count, s->max_elements);
    s->count = count;
    return WDGS_OK;
}
int wdgs_prefix_scanner_scan(wdgs_prefix_scanner* s) {
    WDGS_REQUIRE(s, WDGS_E_INVALID, "null scanner");
    return scan_exclusive_u32(s->dev, &s->scratch, s->input, s->output, s->count, nullptr);
}
int wdgs_prefix_scanner_scan_ptr(wdgs_prefix_scanner* s, const void* in, void* out, uint32_t count) {
    WDGS_REQUIRE(s && in && out, WDGS_E_INVALID, "null argument");
    WDGS_REQUIRE(count <= s->max_elements, WDGS_E_CAPACITY, "scan count %u exceeds max_elements %u", count, s->max_elements);
    return scan_exclusive_u32(s->dev, &s->scratch, static_cast<const u32*>(in), static_cast<u32*>(out), count, nullptr);
}

// ---------------------------------------------------------------- TiledForwardPass
// Tile entries a pass over n Gaussians may produce before it reports WDGS_E_CAPACITY.
static uint64_t forward_tile_entry_cap(const wdgs_tiled_forward_config& cfg, u32 n) {
    uint64_t cap;
    if (cfg.compat_caps) {  // tiled-forward-pass.ts:137-154
        uint64_t base = std::min<uint64_t>((uint64_t)n * 30, (uint64_t)n * 2048);
        cap = std::min<uint64_t>(std::min<uint64_t>(base, 32ull * 1024 * 1024), 2097152ull);
        cap = (cap + 3839) / 3840 * 3840;
    } else if (cfg.max_tile_entries) {
        cap = cfg.max_tile_entries;
    } else {
        cap = std::max<uint64_t>((uint64_t)n * 30, 1ull << 20);
    }
    return std::min<uint64_t>(align_up(cap, 4096), 0xFFFFF000ull);
}
// (Re)allocates the per-Gaussian buffers and the scanner for `capacity` Gaussians: free all, then allocate all
static int forward_alloc_per_point(wdgs_tiled_forward* op, u32 capacity) {
    wdgs_device* d = op->dev;
    op->splats.reset(); op->depths.reset(); op->block_counts.reset(); op->column_counts.reset();
    op->scanner.reset();
    op->points_capacity = 0;
    const size_t blocks = ceil_div(capacity, 256) + 1;
    WDGS_TRY(op->splats.alloc((size_t)6 * capacity, true, d->stream));
    WDGS_TRY(op->depths.alloc(capacity, true, d->stream));
    WDGS_TRY(op->block_counts.alloc(blocks, true, d->stream));
    WDGS_TRY(op->column_counts.alloc(256 * blocks, true, d->stream));
    if (!op->column_totals) WDGS_TRY(op->column_totals.alloc(256, true, d->stream));
    wdgs_prefix_scanner* scanner = nullptr;
    WDGS_TRY(wdgs_prefix_scanner_create(d, capacity, &scanner));
    op->scanner.reset(scanner);
    op->points_capacity = capacity;
    return WDGS_OK;
}
static int forward_make_sorter(wdgs_tiled_forward* op, u32 capacity) {
    wdgs_sorter* sorter = nullptr;
    WDGS_TRY(wdgs_sorter_create(op->dev, capacity, op->stats, &sorter));
    op->sorter.reset(sorter);
    return WDGS_OK;
}
// The settings block and the tile grid the forward kernels are handed, from the host's configuration values (0 = the reference's default) and the
// viewport: what a forward pass builds for itself, and what wdgs_debug_rasterize builds for the frame it is given
static RenderSettings forward_settings(float gaussian_scale, u32 sh_deg, float point_size_px, u32 render_mode, float max_splat_radius_px) {
    return RenderSettings{gaussian_scale != 0.f ? gaussian_scale : 1.0f, (float)sh_deg, 0.f, 0.f, point_size_px != 0.f ? point_size_px : 3.0f,
                          render_mode ? 1.0f : 0.0f, max_splat_radius_px != 0.f ? max_splat_radius_px : 128.0f};
}
static void settings_set_viewport(RenderSettings& st, TileInfo& ti, u32 w, u32 h) {
    st.viewport_x = (float)w;
    st.viewport_y = (float)h;
    ti.num_tiles_x = ceil_div(w, 16);
    ti.num_tiles_y = ceil_div(h, 16);
    ti.total_tiles = ti.num_tiles_x * ti.num_tiles_y;
}
// the sort key keeps tile_id + 1 in 16 bits (tiled-forward.wgsl:121-136)
static bool viewport_tiles_fit(u32 w, u32 h) { return (uint64_t)ceil_div(w, 16) * ceil_div(h, 16) + 1 <= 0xFFFFu; }
static void forward_set_viewport(wdgs_tiled_forward* op, u32 w, u32 h) {
    op->cfg.viewport_width = w;
    op->cfg.viewport_height = h;
    settings_set_viewport(op->settings, op->tile_info, w, h);
}
// The per-tile tables that follow the viewport: the non-finite stamps and, when long lists are on, their marks.  They only grow.
static int forward_alloc_nf_stamp(wdgs_tiled_forward* op) {
    if (op->tile_info.total_tiles <= op->nf_stamp.count()) return WDGS_OK;
    return op->nf_stamp.alloc(op->tile_info.total_tiles, true, op->dev->stream);
}
static int forward_alloc_per_tile(wdgs_tiled_forward* op) {
    const u32 tiles = op->tile_info.total_tiles;
    if (tiles > op->nf_stamp.count()) { (void)wdgs_sync_lanes(op->dev); WDGS_TRY(forward_alloc_nf_stamp(op)); }
    if (op->long_lists.hdr && tiles > op->long_flags.count()) {
        (void)wdgs_sync_lanes(op->dev);
        WDGS_TRY(op->long_flags.alloc(tiles, true, op->dev->stream));
    }
    return WDGS_OK;
}

// The long-list work of a pass lives in ONE device allocation (twelve tables carved out of it: a pass is built inside a densify event, where every
// hipMalloc counts) plus the per-tile marks, which follow the viewport.  `long_lists` is the view of both (and of the stamps) that the kernels are
// handed by value: brought up to date whenever a block it names was re-allocated, and switched off when one of them is not there.
static void forward_sync_long_view(wdgs_tiled_forward* op) {
    LongWork& lw = op->long_lists;
    if (!lw.hdr) return;
    if (!op->long_flags || !op->nf_stamp) { lw = LongWork{}; return; }
    lw.flags = op->long_flags;
    lw.nf_stamp = op->nf_stamp;
}
// (Re)allocates the long-list work of a pass: `threshold` entries (0 = off), room for `items` (block, chunk) slots and `rows` list rows.
static int forward_alloc_long_lists(wdgs_tiled_forward* op, u32 threshold, u32 items, u32 rows) {
    wdgs_device* d = op->dev;
    op->long_base.reset();
    op->long_flags.reset();
    op->long_lists = LongWork{};
    if (threshold == 0u) return WDGS_OK;
    LongWork lw{};
    lw.threshold = threshold;
    lw.max_items = std::max(items, 64u);
    lw.max_blocks = std::max(lw.max_items / 8u, 16u) & ~3u;   // (four per long tile; a tile of `threshold` > 128 entries takes more than 8 items per block)
    lw.max_rows = std::max(rows, 64u);
    const u32 tiles = std::max(op->tile_info.total_tiles, 1u);
    const size_t I = lw.max_items, B = lw.max_blocks, R = lw.max_rows;
    // the small tables first (they are zeroed), the three large ones behind them (written before they are read)
    const size_t sizes[12] = {256, sizeof(LongBlock) * B, sizeof(LongSync) * B, sizeof(u32) * I, sizeof(u32) * I, sizeof(u32) * 64 * B, sizeof(u32) * 64 * B,
                              sizeof(u32) * 64 * I, sizeof(u32) * 64 * I, sizeof(float4) * 192 * I, sizeof(u32) * 256 * R, 0};
    size_t at[12], total = 0, zeroed = 0;
    for (int i = 0; i < 11; i++) { at[i] = total; total += align_up(sizes[i], 256); if (i == 6) zeroed = total; }
    WDGS_TRY(op->long_base.alloc(total, false, d->stream));
    char* const base = op->long_base;
    WDGS_CHECK_HIP(hipMemsetAsync(base, 0, zeroed, d->stream));
    WDGS_TRY(op->long_flags.alloc(tiles, true, d->stream));
    lw.hdr = (u32*)(base + at[0]); lw.blocks = (LongBlock*)(base + at[1]); lw.sync = (LongSync*)(base + at[2]); lw.item_block = (u32*)(base + at[3]); lw.nlist = (u32*)(base + at[4]);
    lw.total = (u32*)(base + at[5]); lw.jlast = (u32*)(base + at[6]); lw.cnt = (u32*)(base + at[7]); lw.off = (u32*)(base + at[8]); lw.records = (float4*)(base + at[9]);
    lw.rows = (u32*)(base + at[10]);
    lw.flags = op->long_flags;
    lw.nf_stamp = op->nf_stamp;
    lw.nf_frame = op->stats + FRAME_WORD;
    op->long_lists = lw;   // (only now: a pass whose allocation failed has its long lists switched off)
    return WDGS_OK;
}
constexpr u32 LONG_LIST_THRESHOLD = 2048u, LONG_LIST_ITEMS = 1024u, LONG_LIST_ROWS = 8192u;   // defaults (include/webdgs.h: wdgs_tiled_forward_set_long_lists)

int wdgs_tiled_forward_create(wdgs_device* d, const wdgs_tiled_forward_config* cfg, wdgs_tiled_forward** out) {
    WDGS_REQUIRE(d && cfg && out, WDGS_E_INVALID, "wdgs_tiled_forward_create: null argument");
    WDGS_REQUIRE(cfg->viewport_width > 0 && cfg->viewport_height > 0, WDGS_E_INVALID, "viewport must be non-empty");
    WDGS_REQUIRE(cfg->sh_deg <= 3, WDGS_E_INVALID, "sh_deg %u > 3", cfg->sh_deg);
    const uint64_t tiles = (uint64_t)ceil_div(cfg->viewport_width, 16) * ceil_div(cfg->viewport_height, 16);
    WDGS_REQUIRE(viewport_tiles_fit(cfg->viewport_width, cfg->viewport_height), WDGS_E_CAPACITY, "%llu tiles do not fit the 16-bit tile field of the sort key", (unsigned long long)tiles);
    auto op = std::make_unique<wdgs_tiled_forward>();
    op->dev = d;
    op->cfg = *cfg;
    const u32 n = cfg->num_points;
    const uint64_t cap = forward_tile_entry_cap(*cfg, n);
    op->settings = forward_settings(cfg->gaussian_scale, cfg->sh_deg, cfg->point_size_px, cfg->render_mode, cfg->max_splat_radius_px);
    op->tile_info.max_tile_entries = (u32)cap;
    forward_set_viewport(op.get(), cfg->viewport_width, cfg->viewport_height);
    WDGS_TRY(op->stats.alloc(FORWARD_STATS_BYTES / 4, true, d->stream));
    // (frame numbers start at 1: a zeroed stamp table marks nothing)
    WDGS_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)(op->stats + FRAME_WORD), 1, 1, d->stream));
    WDGS_TRY(forward_alloc_nf_stamp(op.get()));
    if (!cfg->compat_caps) WDGS_TRY(forward_alloc_long_lists(op.get(), LONG_LIST_THRESHOLD, LONG_LIST_ITEMS, LONG_LIST_ROWS));
    WDGS_CHECK_HIP(hipHostMalloc((void**)&op->host_stats, 16, hipHostMallocDefault));
    std::memset(op->host_stats, 0, 16);
    WDGS_TRY(forward_alloc_per_point(op.get(), std::max(n, 1u)));
    WDGS_TRY(forward_make_sorter(op.get(), (u32)cap));
    d->forwards.push_back(op.get());
    *out = op.release();
    return WDGS_OK;
}

int wdgs_tiled_forward_destroy(wdgs_tiled_forward* op) {
    if (!op) return WDGS_OK;
    if (wdgs_device_alive(op->dev)) {
        auto& v = op->dev->forwards;
        v.erase(std::remove(v.begin(), v.end(), op), v.end());
    }
    sync_if_alive(op->dev);
    if (op->ranges && wdgs_device_alive(op->dev)) op->dev->range_tables.erase(op->ranges.get());
    delete op;
    return WDGS_OK;
}

// The point cloud changed size (densify / prune: applyPointCloudSwap, trainer.ts:201-237, which destroys the pass and builds a new
// one).  Here the pass is kept: its per-Gaussian buffers and its sort buffers are reused when they are large enough and re-allocated
// with 25 % headroom when they are not, so a training run re-allocates a few times at most.  After the call the pass is in the state
// of a freshly created one for n points (zeroed buffers, nothing encoded); max_tile_entries follows the same formula as at creation.
int wdgs_tiled_forward_resize(wdgs_tiled_forward* op, uint32_t n) {
    WDGS_REQUIRE(op, WDGS_E_INVALID, "wdgs_tiled_forward_resize: null op");
    wdgs_device* d = op->dev;
    WDGS_REQUIRE(!d->capturing, WDGS_E_STATE, "wdgs_tiled_forward_resize while recording a command buffer");
    WDGS_CHECK_HIP(hipSetDevice(d->ordinal));
    WDGS_CHECK_HIP(wdgs_sync_lanes(d));
    const u32 need = std::max(n, 1u);
    if (need > op->points_capacity) {
        WDGS_TRY(forward_alloc_per_point(op, (u32)std::min<uint64_t>((uint64_t)need + need / 4, 0xFFFFFFFFull)));
    } else {
        WDGS_CHECK_HIP(hipMemsetAsync(op->splats, 0, (size_t)24 * need, d->stream));
        WDGS_CHECK_HIP(hipMemsetAsync(op->depths, 0, (size_t)4 * need, d->stream));
        WDGS_CHECK_HIP(hipMemsetAsync(op->block_counts, 0, (size_t)4 * (ceil_div(need, 256) + 1), d->stream));
        WDGS_CHECK_HIP(hipMemsetAsync(op->scanner->input, 0, (size_t)4 * need, d->stream));
        WDGS_CHECK_HIP(hipMemsetAsync(op->scanner->output, 0, (size_t)4 * need, d->stream));
    }
    const uint64_t cap = forward_tile_entry_cap(op->cfg, n);
    if (cap > wdgs_sorter_capacity(op->sorter.get())) {
        op->sorter.reset();
        const uint64_t roomy = op->cfg.compat_caps || op->cfg.max_tile_entries ? cap : std::min<uint64_t>(align_up(cap + cap / 4, 4096), 0xFFFFF000ull);
        WDGS_TRY(forward_make_sorter(op, (u32)roomy));
    }
    op->tile_info.max_tile_entries = (u32)cap;
    op->cfg.num_points = n;
    WDGS_CHECK_HIP(hipMemsetAsync(op->stats, 0, 16 + 64 * 4, d->stream));   // (the frame number behind the shards goes on counting)
    std::memset(op->host_stats, 0, 16);
    op->encoded = false;
    op->ranges_valid = false;
    op->projected = false;
    return WDGS_OK;
}

// The tile sort's first pass is folded into its neighbours when the grid allows it (2..256 tile columns, <= 256 tile rows: any
// viewport up to 4096 x 4096): project_count also counts its workgroups' entries per tile COLUMN, the scan kernel turns those into
// per-column offsets, and emit writes its entries straight into column order (project.hip: emit_scatter) -- the keys are never
// written in emission order, histogrammed and scattered.  encode(skipSort) and compat_caps keep the reference's emission order.
static bool forward_uses_columns(const wdgs_tiled_forward* op, int skip_sort) {
    const TileInfo& ti = op->tile_info;
    return !skip_sort && !op->cfg.compat_caps && op->cfg.num_points > 0 && ti.num_tiles_x >= 2u && ti.num_tiles_x <= 256u && ti.num_tiles_y <= 256u;
}

// Everything of TiledForwardPass.encode behind K1: scan (+ stats), emit, sort.
static int forward_encode_rest(wdgs_tiled_forward* op, int skip_sort, bool columns) {
    wdgs_device* d = op->dev;
    const u32 n = op->cfg.num_points;
    const TileInfo& ti = op->tile_info;
    const ScanStatsEpilogue ep{op->stats, op->stats + 4, op->host_stats, op->tile_info.max_tile_entries, op->stats + FRAME_WORD, op->long_lists.hdr};
    if (columns) {
        WDGS_TRY(forward_scan(d, op->block_counts, ceil_div(n, 256), op->column_counts, op->column_totals, ti.num_tiles_x, ep));
    } else if (n > 0) {
        WDGS_TRY(scan_block_sums_inplace(d, op->block_counts, ceil_div(n, 256), ep));
    } else {
        WDGS_TRY(launch_update_stats(d, n, op->scanner->output, op->scanner->input, op->tile_info.max_tile_entries, op->stats, op->stats + 4, op->host_stats));
    }
    op->ranges_valid = false;
    if (!skip_sort && !op->cfg.compat_caps) {
        const u32 tiles = op->tile_info.total_tiles;
        if (tiles + 1 > op->ranges.count()) {
            WDGS_REQUIRE(!d->capturing, WDGS_E_STATE, "TiledForwardPass.encode allocates its range table on first use: run one eager encode before recording");
            (void)wdgs_sync_lanes(d);
            if (op->ranges) d->range_tables.erase(op->ranges.get());
            WDGS_TRY(op->ranges.alloc((size_t)tiles + 1, true, d->stream));
            d->range_tables[op->ranges.get()] = op;   // (a backward pass handed this table finds the pass's long-list work through it)
        }
    }
    u32* const keys0 = static_cast<u32*>(wdgs_sorter_keys(op->sorter.get(), 0));   // emit writes the entries into ping-pong 0
    u32* const values0 = static_cast<u32*>(wdgs_sorter_values(op->sorter.get(), 0));
    if (columns) {
        WDGS_TRY(launch_emit_scatter(d, n, op->splats, op->depths, op->scanner->input, op->scanner->output, op->block_counts, op->settings, op->tile_info,
                                     op->column_counts, op->column_totals, keys0, values0, op->tile_info.max_tile_entries));
        // one stable pass on the tile row (it builds the range table), then the per-tile depth sort: the order of a stable sort of the full key
        WDGS_TRY(sorter_sort_rows(op->sorter.get(), ti.num_tiles_x, ti.num_tiles_y, op->ranges, op->long_lists.hdr ? &op->long_lists : nullptr));
        op->ranges_valid = true;
    } else {
        WDGS_TRY(launch_emit(d, n, op->splats, op->depths, op->scanner->input, op->scanner->output, op->block_counts, op->settings, op->tile_info, keys0, values0,
                             op->tile_info.max_tile_entries));
        if (skip_sort) sorter_set_final_out_index(op->sorter.get(), 0);  // the unsorted entries are in ping-pong 0
        if (!skip_sort) {
            // key = (tile_id + 1) << 16 | depth16: only 16 + bits(total_tiles) bits are ever set
            if (op->cfg.compat_caps) {
                WDGS_TRY(wdgs_sorter_sort(op->sorter.get(), 32u));  // the reference's four 8-bit passes over the whole key
            } else {
                // tile passes, range table, per-tile depth sort (sort.hip): the order of a stable sort of the full key
                WDGS_TRY(sorter_sort_segmented(op->sorter.get(), bits_for(op->tile_info.total_tiles), op->tile_info.total_tiles, op->ranges, op->long_lists.hdr ? &op->long_lists : nullptr));
                op->ranges_valid = true;
            }
        }
    }
    op->encoded = true;
    return WDGS_OK;
}

int wdgs_tiled_forward_encode(wdgs_tiled_forward* op, const void* gaussians, const void* sh, const void* camera, int skip_sort) {
    WDGS_REQUIRE(op && gaussians && sh && camera, WDGS_E_INVALID, "wdgs_tiled_forward_encode: null argument");
    wdgs_device* d = op->dev;
    const u32 n = op->cfg.num_points;
    // clearBuffer(pipelineStatsBuffer) (tiled-forward-pass.ts:345) needs no launch here: update_stats overwrites words 0..2, word 3
    // stays 0, and the visible count is accumulated in shard words that update_stats clears after folding them.
    // The offsets scan (K2-K4) is spread over its neighbours: project_count leaves the entry count of each of its workgroups, one
    // single-workgroup kernel scans those N/256 sums (and publishes the stats block: update_stats, K5, as its epilogue), and emit adds
    // its own in-workgroup prefix -- writing the per-Gaussian offsets table on the way.  Three launches instead of five.
    const bool columns = forward_uses_columns(op, skip_sort);
    op->projected = false;  // (K1 overwrites whatever projection the buffers held)
    WDGS_TRY(launch_project_count(d, n, static_cast<const u32*>(gaussians), static_cast<const u32*>(sh), static_cast<const float*>(camera), op->settings, op->tile_info,
                                  op->splats, op->depths, op->scanner->input, op->stats + 4, op->block_counts, columns ? op->column_counts : nullptr, op->dc_source,
                                  op->nf_stamp, op->stats + FRAME_WORD));
    return forward_encode_rest(op, skip_sort, columns);
}

// ---- view-batched K1 (include/webdgs.h)
int wdgs_tiled_forward_project_views(wdgs_tiled_forward* const* ops, const void* const* cameras, uint32_t count, const void* gaussians, const void* sh) {
    WDGS_REQUIRE(ops && cameras && gaussians && sh && count > 0 && count <= WDGS_MAX_BATCH_VIEWS, WDGS_E_INVALID, "wdgs_tiled_forward_project_views: invalid argument");
    wdgs_tiled_forward* f0 = ops[0];
    WDGS_REQUIRE(f0, WDGS_E_INVALID, "wdgs_tiled_forward_project_views: null pass");
    const bool columns = forward_uses_columns(f0, 0);
    ProjectViews pv{count};
    for (u32 v = 0; v < count; v++) {
        wdgs_tiled_forward* f = ops[v];
        WDGS_REQUIRE(f && cameras[v], WDGS_E_INVALID, "wdgs_tiled_forward_project_views: null pass or camera %u", v);
        for (u32 u = 0; u < v; u++) WDGS_REQUIRE(ops[u] != f, WDGS_E_INVALID, "wdgs_tiled_forward_project_views: pass %u is given twice (every view needs buffers of its own)", v);
        WDGS_REQUIRE(f->dev == f0->dev && f->cfg.num_points == f0->cfg.num_points && f->cfg.sh_deg == f0->cfg.sh_deg && f->cfg.compat_caps == f0->cfg.compat_caps &&
                         std::memcmp(&f->settings, &f0->settings, sizeof(RenderSettings)) == 0 && f->tile_info.num_tiles_x == f0->tile_info.num_tiles_x &&
                         f->tile_info.num_tiles_y == f0->tile_info.num_tiles_y && f->dc_source == f0->dc_source,
                     WDGS_E_STATE, "wdgs_tiled_forward_project_views: pass %u differs from pass 0 (cloud size, SH degree, viewport, settings or dc source)", v);
        pv.camera[v] = static_cast<const float*>(cameras[v]); pv.splats[v] = f->splats; pv.depths[v] = f->depths; pv.tile_counts[v] = f->scanner->input;
        pv.visible_shards[v] = f->stats + 4; pv.block_counts[v] = f->block_counts; pv.column_counts[v] = columns ? f->column_counts.get() : nullptr;
        pv.nf_stamp[v] = f->nf_stamp; pv.nf_frame[v] = f->stats + FRAME_WORD;
    }
    WDGS_TRY(launch_project_count_views(f0->dev, f0->cfg.num_points, static_cast<const u32*>(gaussians), static_cast<const u32*>(sh), f0->settings, f0->tile_info, pv,
                                        f0->dc_source));
    for (u32 v = 0; v < count; v++) { ops[v]->projected = true; ops[v]->projected_columns = columns; }
    return WDGS_OK;
}
int wdgs_tiled_forward_encode_projected(wdgs_tiled_forward* op) {
    WDGS_REQUIRE(op, WDGS_E_INVALID, "wdgs_tiled_forward_encode_projected: null op");
    if (op->dev->capturing) {
        // recorded: nothing runs now, so nothing is consumed now -- every submit of the command buffer will need (and use up) a projection
        // of this pass (wdgs_queue_submit).  Whether the columns were counted is a property of the pass's configuration, not of one projection.
        op->dev->capture_consumes.push_back(op);
        return forward_encode_rest(op, 0, forward_uses_columns(op, 0));
    }
    WDGS_REQUIRE(op->projected, WDGS_E_STATE,
                 "wdgs_tiled_forward_encode_projected: the pass holds no projection (wdgs_tiled_forward_project_views), or a later encode has consumed or overwritten it");
    op->projected = false;  // the scan consumes K1's workgroup sums in place: the rest of the pass can run ONCE per projection
    return forward_encode_rest(op, 0, op->projected_columns);
}
static bool forward_holds_projection(const wdgs_tiled_forward* f) { return f->projected; }
static void forward_consume_projection(wdgs_tiled_forward* f) { f->projected = false; }

int wdgs_tiled_forward_is_projected(const wdgs_tiled_forward* op) { return (op && op->projected) ? 1 : 0; }

int wdgs_tiled_forward_set_viewport(wdgs_tiled_forward* op, uint32_t w, uint32_t h) {
    WDGS_REQUIRE(op && w > 0 && h > 0, WDGS_E_INVALID, "wdgs_tiled_forward_set_viewport: invalid argument");
    WDGS_REQUIRE(viewport_tiles_fit(w, h), WDGS_E_CAPACITY, "viewport %ux%u has too many tiles for the 16-bit tile field", w, h);
    WDGS_REQUIRE(!op->dev->capturing, WDGS_E_STATE, "wdgs_tiled_forward_set_viewport while recording a command buffer");
    forward_set_viewport(op, w, h);
    const int r = forward_alloc_per_tile(op);
    forward_sync_long_view(op);   // (after a failure too: the view never names a block that has been freed)
    return r;
}
int wdgs_tiled_forward_set_render_mode(wdgs_tiled_forward* op, uint32_t mode) {
    WDGS_REQUIRE(op, WDGS_E_INVALID, "null op");
    op->cfg.render_mode = mode;
    op->settings.gaussian_mode = mode ? 1.0f : 0.0f;
    return WDGS_OK;
}
int wdgs_tiled_forward_set_point_size(wdgs_tiled_forward* op, float v) {
    WDGS_REQUIRE(op, WDGS_E_INVALID, "null op");
    op->settings.point_size_px = v;
    return WDGS_OK;
}
int wdgs_tiled_forward_set_gaussian_scale(wdgs_tiled_forward* op, float v) {
    WDGS_REQUIRE(op, WDGS_E_INVALID, "null op");
    op->settings.gaussian_scaling = v;
    return WDGS_OK;
}

int wdgs_tiled_forward_get_resources(wdgs_tiled_forward* op, wdgs_tiled_forward_resources* out) {
    WDGS_REQUIRE(op && out, WDGS_E_INVALID, "null argument");
    const int fo = wdgs_sorter_final_out_index(op->sorter.get());
    out->splat_buffer = op->splats;
    out->depths_buffer = op->depths;
    out->tile_keys_buffer = wdgs_sorter_keys(op->sorter.get(), fo);
    out->tile_indices_buffer = wdgs_sorter_values(op->sorter.get(), fo);
    out->tile_offsets_buffer = op->scanner->output;
    out->tile_counts_buffer = op->scanner->input;
    out->stats_buffer = op->stats;
    out->num_tiles_x = op->tile_info.num_tiles_x;
    out->num_tiles_y = op->tile_info.num_tiles_y;
    out->total_tiles = op->tile_info.total_tiles;
    out->max_tile_entries = op->tile_info.max_tile_entries;
    std::memcpy(out->settings, &op->settings, sizeof(float) * 7);
    return WDGS_OK;
}

int wdgs_tiled_forward_check(wdgs_tiled_forward* op, uint32_t* stats_out) {
    WDGS_REQUIRE(op, WDGS_E_INVALID, "null op");
    WDGS_REQUIRE(!op->dev->capturing, WDGS_E_STATE, "wdgs_tiled_forward_check while recording a command buffer");
    WDGS_CHECK_HIP(wdgs_sync_lanes(op->dev));
    u32 st[4];
    for (int i = 0; i < 4; i++) st[i] = ((const volatile u32*)op->host_stats)[i];
    st[2] = __atomic_exchange_n(op->host_stats + 2, 0u, __ATOMIC_ACQ_REL);  // the overflow word is sticky (set by any encode since the last check): consumed here, atomically
    if (stats_out) std::memcpy(stats_out, st, sizeof(st));
    WDGS_REQUIRE(st[2] == 0u, WDGS_E_CAPACITY, "tile entries overflow: %u entries needed, max_tile_entries = %u (forward pass %p)", st[2], op->tile_info.max_tile_entries, (void*)op);
    return WDGS_OK;
}

int wdgs_tiled_forward_set_long_lists(wdgs_tiled_forward* op, uint32_t threshold, uint32_t max_items, uint32_t max_rows) {
    WDGS_REQUIRE(op, WDGS_E_INVALID, "wdgs_tiled_forward_set_long_lists: null op");
    wdgs_device* d = op->dev;
    WDGS_REQUIRE(!d->capturing, WDGS_E_STATE, "wdgs_tiled_forward_set_long_lists while recording a command buffer");
    WDGS_REQUIRE(!op->cfg.compat_caps || threshold == 0u, WDGS_E_STATE, "wdgs_tiled_forward_set_long_lists: a pass with compat_caps truncates its lists as the reference does");
    WDGS_CHECK_HIP(hipSetDevice(d->ordinal));
    WDGS_CHECK_HIP(wdgs_sync_lanes(d));
    const LongWork& now = op->long_lists;
    return forward_alloc_long_lists(op, threshold, max_items ? max_items : (now.hdr ? now.max_items : LONG_LIST_ITEMS), max_rows ? max_rows : (now.hdr ? now.max_rows : LONG_LIST_ROWS));
}
int wdgs_tiled_forward_long_list_stats(wdgs_tiled_forward* op, uint32_t stats_out[12]) {
    WDGS_REQUIRE(op && stats_out, WDGS_E_INVALID, "wdgs_tiled_forward_long_list_stats: null argument");
    std::memset(stats_out, 0, sizeof(uint32_t) * 12);
    const LongWork& lw = op->long_lists;
    if (!lw.hdr) return WDGS_OK;
    WDGS_TRY(wdgs_copy_to_host(op->dev, stats_out, lw.hdr, sizeof(u32) * LL_HDR_WORDS));
    stats_out[8] = lw.max_items; stats_out[9] = lw.max_blocks; stats_out[10] = lw.max_rows; stats_out[11] = lw.threshold;
    return WDGS_OK;
}

// ---------------------------------------------------------------- TiledRasterizer
int wdgs_tiled_rasterizer_create(wdgs_device* d, wdgs_tiled_forward* fwd, uint32_t compat_caps, wdgs_tiled_rasterizer** out) {
    WDGS_REQUIRE(d && fwd && out, WDGS_E_INVALID, "wdgs_tiled_rasterizer_create: null argument");
    auto op = std::make_unique<wdgs_tiled_rasterizer>();
    op->dev = d;
    op->fwd = fwd;
    op->compat_caps = compat_caps;
    *out = op.release();
    return WDGS_OK;
}
int wdgs_tiled_rasterizer_destroy(wdgs_tiled_rasterizer* op) {
    if (!op) return WDGS_OK;
    sync_if_alive(op->dev);
    delete op;
    return WDGS_OK;
}
// The frame op's last encode composited (or is about to: op->ranges_used is set), as the walkers of its tile lists take it (launch.h)
static CompositedFrame composited_frame(const wdgs_tiled_rasterizer* op) {
    const wdgs_tiled_forward* f = op->fwd;
    const int fo = wdgs_sorter_final_out_index(f->sorter.get());
    return CompositedFrame{f->settings, f->tile_info, f->splats, f->cfg.num_points, op->ranges_used, static_cast<const u32*>(wdgs_sorter_keys(f->sorter.get(), fo)),
                           static_cast<const u32*>(wdgs_sorter_values(f->sorter.get(), fo)), f->stats, op->compat_caps ? 32u : 0u, f->nf_stamp, f->stats + FRAME_WORD};
}
// What encodeDepth and encodeContribution (`what`) need of the last encode: that there was one, of the viewport the forward pass still has, in Gaussian mode
static int require_composited_frame(const wdgs_tiled_rasterizer* op, const char* what) {
    const wdgs_tiled_forward* f = op->fwd;
    WDGS_REQUIRE(op->encoded && f->encoded && op->ranges_used, WDGS_E_STATE, "TiledRasterizer.%s before encode: it composites the frame encode rasterized", what);
    WDGS_REQUIRE(op->width == f->cfg.viewport_width && op->height == f->cfg.viewport_height, WDGS_E_STATE,
                 "TiledRasterizer.%s: the forward pass viewport changed to %ux%u since the last encode (%ux%u)", what, f->cfg.viewport_width, f->cfg.viewport_height,
                 op->width, op->height);
    WDGS_REQUIRE(f->settings.gaussian_mode >= 0.5f, WDGS_E_STATE, "TiledRasterizer.%s: the forward pass is in point-cloud render mode, which has no weights", what);
    return WDGS_OK;
}
int wdgs_tiled_rasterizer_encode(wdgs_tiled_rasterizer* op, uint32_t width, uint32_t height) {
    WDGS_REQUIRE(op && width > 0 && height > 0, WDGS_E_INVALID, "wdgs_tiled_rasterizer_encode: invalid argument");
    wdgs_tiled_forward* f = op->fwd;
    WDGS_REQUIRE(f->encoded, WDGS_E_STATE, "rasterizer encode before the forward pass was encoded");
    WDGS_REQUIRE(width == f->cfg.viewport_width && height == f->cfg.viewport_height, WDGS_E_STATE,
                 "rasterizer size %ux%u differs from the forward pass viewport %ux%u", width, height, f->cfg.viewport_width, f->cfg.viewport_height);
    wdgs_device* d = op->dev;
    const TileInfo& ti = f->tile_info;
    if (width != op->width || height != op->height) {  // ensureTextures (tiled-rasterizer.ts:244-306)
        WDGS_REQUIRE(!d->capturing, WDGS_E_STATE, "TiledRasterizer.encode allocates its textures on first use: run one eager encode before recording");
        (void)wdgs_sync_lanes(d);
        op->rgba8.reset(); op->alpha.reset(); op->n_contrib.reset();   // free all, then allocate all
        op->width = op->height = 0;   // (the size of the images the pass HOLDS: none until all three are there)
        const size_t px = (size_t)width * height;
        WDGS_TRY(op->rgba8.alloc(px, true, d->stream));
        WDGS_TRY(op->alpha.alloc(px, true, d->stream));
        WDGS_TRY(op->n_contrib.alloc(px, true, d->stream));
        op->width = width;
        op->height = height;
    }
    const int fo = wdgs_sorter_final_out_index(f->sorter.get());
    const u32* keys = static_cast<const u32*>(wdgs_sorter_keys(f->sorter.get(), fo));
    if (f->ranges_valid) {
        op->ranges_used = f->ranges;  // built by the forward pass's sort
    } else {
        if (ti.total_tiles + 1 > op->ranges.count()) {
            WDGS_REQUIRE(!d->capturing, WDGS_E_STATE, "TiledRasterizer.encode allocates its range table on first use: run one eager encode before recording");
            (void)wdgs_sync_lanes(d);
            op->ranges_used = nullptr;
            WDGS_TRY(op->ranges.alloc((size_t)ti.total_tiles + 1, true, d->stream));
        }
        WDGS_TRY(launch_tile_ranges(d, keys, f->stats, ti.total_tiles, op->ranges));
        op->ranges_used = op->ranges;
    }
    WDGS_TRY(launch_rasterize(d, composited_frame(op), op->rgba8, op->alpha, op->n_contrib,
                              (f->ranges_valid && f->long_lists.hdr && !op->compat_caps) ? &f->long_lists : nullptr));   // (the table this pass's sort built and marked)
    op->encoded = true;
    return WDGS_OK;
}

// Test hook (include/webdgs.h): launch_rasterize on a CompositedFrame made of the caller's device pointers -- the settings block and the tile grid
// by the forward pass's own forward_settings / settings_set_viewport, the launch by the call wdgs_tiled_rasterizer_encode makes, without the
// long-list work.  The walkers of tilewalk.h take the same struct: a hook for them would build its frame here too.
static int debug_frame(const wdgs_debug_raster_frame* fr, const char* who, CompositedFrame* out) {
    WDGS_REQUIRE(fr->splats && fr->sorted_keys && fr->sorted_vals && fr->count && fr->ranges, WDGS_E_INVALID, "%s: null table in the frame", who);
    WDGS_REQUIRE(fr->viewport_width > 0 && fr->viewport_height > 0, WDGS_E_INVALID, "%s: the viewport must be non-empty, not %u x %u", who, fr->viewport_width,
                 fr->viewport_height);
    WDGS_REQUIRE(viewport_tiles_fit(fr->viewport_width, fr->viewport_height), WDGS_E_INVALID, "%s: viewport %ux%u has too many tiles for the 16-bit tile field", who,
                 fr->viewport_width, fr->viewport_height);
    WDGS_REQUIRE(!fr->nf_stamp || fr->nf_frame, WDGS_E_INVALID, "%s: nf_stamp without the frame word it is compared with", who);
    CompositedFrame f = {};
    f.st = forward_settings(0.f, 0u, fr->point_size_px, fr->render_mode, fr->max_splat_radius_px);
    settings_set_viewport(f.st, f.ti, fr->viewport_width, fr->viewport_height);
    f.splats = static_cast<const u32*>(fr->splats);
    f.num_splats = fr->num_splats;
    f.ranges = static_cast<const u32*>(fr->ranges);
    f.sorted_keys = static_cast<const u32*>(fr->sorted_keys);
    f.sorted_vals = static_cast<const u32*>(fr->sorted_vals);
    f.count_ptr = static_cast<const u32*>(fr->count);
    f.max_batches = fr->max_batches;
    f.nf_stamp = static_cast<const u32*>(fr->nf_stamp);
    f.nf_frame = static_cast<const u32*>(fr->nf_frame);
    *out = f;
    return WDGS_OK;
}
int wdgs_debug_rasterize(wdgs_device* dev, const wdgs_debug_raster_frame* frame, void* rgba8_dev, void* final_t_dev, void* n_contrib_dev) {
    WDGS_REQUIRE(dev && frame && rgba8_dev && final_t_dev && n_contrib_dev, WDGS_E_INVALID, "wdgs_debug_rasterize: null argument");
    CompositedFrame f;
    WDGS_TRY(debug_frame(frame, "wdgs_debug_rasterize", &f));
    return launch_rasterize(dev, f, static_cast<u32*>(rgba8_dev), static_cast<float*>(final_t_dev), static_cast<u32*>(n_contrib_dev), nullptr);
}

// Depth images of the frame the last encode composited (depth.hip; no counterpart in the reference, which renders colour only).  The walk is
// launch_rasterize's without the long-list work (tilewalk.h): the same CompositedFrame, plus the forward pass's depth words.
int wdgs_tiled_rasterizer_encode_depth(wdgs_tiled_rasterizer* op, uint32_t kinds) {
    WDGS_REQUIRE(op, WDGS_E_INVALID, "wdgs_tiled_rasterizer_encode_depth: null op");
    constexpr uint32_t all = WDGS_DEPTH_EXPECTED | WDGS_DEPTH_MEDIAN | WDGS_DEPTH_WEIGHT_SUM;
    WDGS_REQUIRE(kinds != 0u && (kinds & ~all) == 0u, WDGS_E_INVALID, "wdgs_tiled_rasterizer_encode_depth: kinds 0x%x is not a non-empty set of WDGS_DEPTH_* bits", kinds);
    WDGS_TRY(require_composited_frame(op, "encodeDepth"));
    wdgs_device* d = op->dev;
    if (op->depth_width != op->width || op->depth_height != op->height) {   // a size change: the images are re-made per kind below
        bool any = false;
        for (const DevMem<float>& img : op->depth) any = any || img;
        if (any) {
            WDGS_REQUIRE(!d->capturing, WDGS_E_STATE, "TiledRasterizer.encodeDepth re-allocates its images after a size change: run one eager encodeDepth before recording");
            (void)wdgs_sync_lanes(d);
            for (DevMem<float>& img : op->depth) img.reset();
        }
        op->depth_width = op->width;
        op->depth_height = op->height;
    }
    for (u32 k = 0; k < 3u; k++) {
        if (!((kinds >> k) & 1u) || op->depth[k]) continue;
        WDGS_REQUIRE(!d->capturing, WDGS_E_STATE, "TiledRasterizer.encodeDepth allocates a depth image on first use of its kind: run one eager encodeDepth before recording");
        WDGS_TRY(op->depth[k].alloc((size_t)op->width * op->height, true, d->stream));
    }
    WDGS_TRY(launch_depth_composite(d, composited_frame(op), op->fwd->depths, (kinds & WDGS_DEPTH_WEIGHT_SUM) ? op->depth[2] : nullptr,
                                    (kinds & WDGS_DEPTH_EXPECTED) ? op->depth[0] : nullptr, (kinds & WDGS_DEPTH_MEDIAN) ? op->depth[1] : nullptr));
    op->depth_encoded = kinds;
    return WDGS_OK;
}
// Per-Gaussian contribution of the frame the last encode composited (contrib.hip; no counterpart in the reference).  depth's walk and arguments without
// the depth words; the records are the caller's, added to, and nothing is allocated: the call records.
int wdgs_tiled_rasterizer_encode_contribution(wdgs_tiled_rasterizer* op, void* stats_dev) {
    WDGS_REQUIRE(op, WDGS_E_INVALID, "wdgs_tiled_rasterizer_encode_contribution: null op");
    WDGS_REQUIRE(stats_dev && ((uintptr_t)stats_dev & 15u) == 0u, WDGS_E_INVALID,
                 "wdgs_tiled_rasterizer_encode_contribution: the statistics buffer must be non-null and 16-byte aligned (got %p)", stats_dev);
    WDGS_TRY(require_composited_frame(op, "encodeContribution"));
    return launch_contribution(op->dev, composited_frame(op), stats_dev);
}
// Normal map of the frame the last encode composited (normal.hip; no counterpart in the reference): the per-Gaussian words from the cloud and the camera
// the forward pass was encoded with -- the caller's, as in wdgs_tiled_forward_encode, which keeps neither -- then depth's walk over them.  The words and the
// image are allocated at first use, under the depth images' rules.
int wdgs_tiled_rasterizer_encode_normal(wdgs_tiled_rasterizer* op, const void* gaussians, const void* camera) {
    WDGS_REQUIRE(op && gaussians && camera, WDGS_E_INVALID, "wdgs_tiled_rasterizer_encode_normal: null argument");
    WDGS_TRY(require_composited_frame(op, "encodeNormal"));
    wdgs_device* d = op->dev;
    const u32 n = op->fwd->cfg.num_points;
    if (!op->normals || op->normals_points != n) {   // first use, or the point count changed: the words are re-made
        WDGS_REQUIRE(!d->capturing, WDGS_E_STATE, "TiledRasterizer.encodeNormal allocates its per-Gaussian normals on first use and after a point-count change: run one eager encodeNormal before recording");
        if (op->normals) (void)wdgs_sync_lanes(d);
        op->normals_points = 0;
        op->normal_encoded = false;
        WDGS_TRY(op->normals.alloc(std::max(n, 1u), true, d->stream));
        op->normals_points = n;
    }
    if (!op->normal_image || op->normal_width != op->width || op->normal_height != op->height) {
        WDGS_REQUIRE(!d->capturing, WDGS_E_STATE, "TiledRasterizer.encodeNormal allocates its image on first use and after a size change: run one eager encodeNormal before recording");
        if (op->normal_image) (void)wdgs_sync_lanes(d);
        op->normal_width = op->normal_height = 0;
        op->normal_encoded = false;
        WDGS_TRY(op->normal_image.alloc((size_t)op->width * op->height, true, d->stream));
        op->normal_width = op->width;
        op->normal_height = op->height;
    }
    WDGS_TRY(launch_gaussian_normals(d, n, static_cast<const u32*>(gaussians), static_cast<const float*>(camera), op->normals));
    WDGS_TRY(launch_normal_composite(d, composited_frame(op), op->normals, op->normal_image));
    op->normal_encoded = true;
    return WDGS_OK;
}
int wdgs_tiled_rasterizer_get_normal(wdgs_tiled_rasterizer* op, void** out) {
    WDGS_REQUIRE(op && out, WDGS_E_INVALID, "wdgs_tiled_rasterizer_get_normal: null argument");
    WDGS_REQUIRE(op->normal_encoded && op->normal_image, WDGS_E_STATE, "TiledRasterizer: normal image not encoded yet (call encodeNormal first)");
    WDGS_REQUIRE(op->normal_width == op->width && op->normal_height == op->height, WDGS_E_STATE,
                 "TiledRasterizer: the normal image is %ux%u, the rasterizer's images %ux%u since the last encode (call encodeNormal again)", op->normal_width, op->normal_height,
                 op->width, op->height);
    *out = op->normal_image;
    return WDGS_OK;
}
int wdgs_tiled_rasterizer_get_gaussian_normals(wdgs_tiled_rasterizer* op, void** out) {
    WDGS_REQUIRE(op && out, WDGS_E_INVALID, "wdgs_tiled_rasterizer_get_gaussian_normals: null argument");
    WDGS_REQUIRE(op->normal_encoded && op->normals, WDGS_E_STATE, "TiledRasterizer: per-Gaussian normals not encoded yet (call encodeNormal first)");
    // (the rasterizer is not told of a resize of the forward pass: the words of another point count are not handed out -- the next encode_normal re-makes them)
    WDGS_REQUIRE(op->normals_points == op->fwd->cfg.num_points, WDGS_E_STATE,
                 "TiledRasterizer: the per-Gaussian normals hold %u Gaussians, the forward pass %u since its point count changed (call encodeNormal again)", op->normals_points,
                 op->fwd->cfg.num_points);
    *out = op->normals;
    return WDGS_OK;
}
int wdgs_tiled_rasterizer_get_depth(wdgs_tiled_rasterizer* op, uint32_t kind, void** out) {
    WDGS_REQUIRE(op && out, WDGS_E_INVALID, "wdgs_tiled_rasterizer_get_depth: null argument");
    WDGS_REQUIRE(kind == WDGS_DEPTH_EXPECTED || kind == WDGS_DEPTH_MEDIAN || kind == WDGS_DEPTH_WEIGHT_SUM, WDGS_E_INVALID,
                 "wdgs_tiled_rasterizer_get_depth: kind 0x%x is not one WDGS_DEPTH_* bit", kind);
    const u32 k = kind == WDGS_DEPTH_EXPECTED ? 0u : kind == WDGS_DEPTH_MEDIAN ? 1u : 2u;
    WDGS_REQUIRE((op->depth_encoded & kind) && op->depth[k], WDGS_E_STATE, "TiledRasterizer: depth image of this kind not encoded yet (call encodeDepth with it first)");
    *out = op->depth[k];
    return WDGS_OK;
}
#define RASTER_GETTER(fn, field, what)                                                                            \
    int fn(wdgs_tiled_rasterizer* op, void** out) {                                                               \
        WDGS_REQUIRE(op && out, WDGS_E_INVALID, #fn ": null argument");                                           \
        WDGS_REQUIRE(op->encoded && op->field, WDGS_E_STATE, "TiledRasterizer: " what " not created yet (call encode first)"); \
        *out = op->field;                                                                                         \
        return WDGS_OK;                                                                                           \
    }
RASTER_GETTER(wdgs_tiled_rasterizer_get_output, rgba8, "output texture")
RASTER_GETTER(wdgs_tiled_rasterizer_get_alpha, alpha, "alpha texture")
RASTER_GETTER(wdgs_tiled_rasterizer_get_n_contrib, n_contrib, "n_contrib texture")
RASTER_GETTER(wdgs_tiled_rasterizer_get_tile_offsets, ranges_used, "tile offsets")
#undef RASTER_GETTER

int wdgs_tiled_rasterizer_blit(wdgs_tiled_rasterizer* op, void* target, uint32_t tw, uint32_t th) {
    WDGS_REQUIRE(op && target, WDGS_E_INVALID, "wdgs_tiled_rasterizer_blit: null argument");
    WDGS_REQUIRE(op->encoded && op->rgba8, WDGS_E_STATE, "TiledRasterizer: no output texture to blit from. Call encode() first.");
    WDGS_REQUIRE(tw > 0 && th > 0, WDGS_E_INVALID, "wdgs_tiled_rasterizer_blit: empty target %ux%u", tw, th);
    return launch_downsample(op->dev, op->rgba8, op->width, op->height, static_cast<u32*>(target), tw, th);
}

// ---------------------------------------------------------------- TiledBackwardPass
static int backward_alloc_images(wdgs_tiled_backward* op, u32 w, u32 h) {
    const u32 px = w * h;
    if (px <= op->metric_flags.count()) return WDGS_OK;   // (the image allocated last: when it is there, all three are)
    hipStream_t stream = op->dev->stream;
    (void)wdgs_sync_lanes(op->dev);
    op->loss_image.reset(); op->metric_err.reset(); op->metric_flags.reset();   // free all, then allocate all
    WDGS_TRY(op->loss_image.alloc(px, true, stream));
    WDGS_TRY(op->metric_err.alloc(px, true, stream));
    WDGS_TRY(op->metric_flags.alloc(px, true, stream));
    return WDGS_OK;
}

// (Re)allocates the per-Gaussian buffers for `capacity` Gaussians: free all, then allocate all
static int backward_alloc_per_point(wdgs_tiled_backward* op, u32 capacity) {
    hipStream_t stream = op->dev->stream;
    op->acc.reset(); op->gradients.reset(); op->metric_counts.reset();
    op->points_capacity = 0;
    WDGS_TRY(op->acc.alloc((size_t)capacity * 12 + 4, true, stream));
    WDGS_TRY(op->gradients.alloc((size_t)capacity * 8, true, stream));
    WDGS_TRY(op->metric_counts.alloc(capacity, true, stream));
    op->points_capacity = capacity;
    return WDGS_OK;
}
// Counterpart of wdgs_tiled_forward_resize for the backward pass's per-Gaussian buffers (accumulators, packed gradients, metric counts).
int wdgs_tiled_backward_resize(wdgs_tiled_backward* op, uint32_t n) {
    WDGS_REQUIRE(op, WDGS_E_INVALID, "wdgs_tiled_backward_resize: null op");
    wdgs_device* d = op->dev;
    WDGS_REQUIRE(!d->capturing, WDGS_E_STATE, "wdgs_tiled_backward_resize while recording a command buffer");
    WDGS_CHECK_HIP(hipSetDevice(d->ordinal));
    WDGS_CHECK_HIP(wdgs_sync_lanes(d));
    const u32 need = std::max(n, 1u);
    if (need > op->points_capacity) {
        WDGS_TRY(backward_alloc_per_point(op, (u32)std::min<uint64_t>((uint64_t)need + need / 4, 0xFFFFFFFFull)));
    } else {
        WDGS_CHECK_HIP(hipMemsetAsync(op->acc, 0, (size_t)need * 48, d->stream));
        WDGS_CHECK_HIP(hipMemsetAsync(op->acc_dirty(), 0, 16, d->stream));
        WDGS_CHECK_HIP(hipMemsetAsync(op->gradients, 0, (size_t)need * 32, d->stream));
        WDGS_CHECK_HIP(hipMemsetAsync(op->metric_counts, 0, (size_t)need * 4, d->stream));
    }
    op->cfg.num_points = n;
    return WDGS_OK;
}
int wdgs_tiled_backward_create(wdgs_device* d, const wdgs_tiled_backward_config* cfg, wdgs_tiled_backward** out) {
    WDGS_REQUIRE(d && cfg && out, WDGS_E_INVALID, "wdgs_tiled_backward_create: null argument");
    WDGS_REQUIRE(cfg->viewport_width > 0 && cfg->viewport_height > 0, WDGS_E_INVALID, "viewport must be non-empty");
    auto op = std::make_unique<wdgs_tiled_backward>();
    op->dev = d;
    op->cfg = *cfg;
    if (op->cfg.training.c1 == 0.f) op->cfg.training.c1 = 0.01f * 0.01f;  // tiled-backward-pass.ts:172-173
    if (op->cfg.training.c2 == 0.f) op->cfg.training.c2 = 0.03f * 0.03f;
    op->settings = RenderSettings{cfg->gaussian_scale != 0.f ? cfg->gaussian_scale : 1.0f, (float)cfg->sh_deg, (float)cfg->viewport_width,
                                  (float)cfg->viewport_height, cfg->point_size_px != 0.f ? cfg->point_size_px : 3.0f, 0.0f,
                                  cfg->max_splat_radius_px != 0.f ? cfg->max_splat_radius_px : 128.0f};
    WDGS_TRY(backward_alloc_per_point(op.get(), std::max(cfg->num_points, 1u)));
    WDGS_TRY(op->metric_minmax.alloc(1024, true, d->stream));
    WDGS_TRY(backward_alloc_images(op.get(), cfg->viewport_width, cfg->viewport_height));
    *out = op.release();
    return WDGS_OK;
}
int wdgs_tiled_backward_destroy(wdgs_tiled_backward* op) {
    if (!op) return WDGS_OK;
    sync_if_alive(op->dev);
    delete op;
    return WDGS_OK;
}
int wdgs_tiled_backward_set_gradient_output(wdgs_tiled_backward* op, int enabled) {
    WDGS_REQUIRE(op, WDGS_E_INVALID, "wdgs_tiled_backward_set_gradient_output: null op");
    op->gradient_output = enabled != 0;
    return WDGS_OK;
}
// K15, the loss image of the pass's loss (dssim_mode): the reference's heuristic (loss.hip) or the exact D-SSIM gradient (dssim.hip); both clear
// the accumulators when acc is given and they are dirty
static int backward_loss(wdgs_tiled_backward* op, const void* pred, const void* targ, int* acc, u32 acc_rows, const u32* acc_dirty) {
    const u32 w = op->cfg.viewport_width, h = op->cfg.viewport_height;
    const auto launch = op->dssim_mode == WDGS_DSSIM_GAUSSIAN ? launch_dssim_grad : launch_loss_grad;
    return launch(op->dev, w, h, static_cast<const u32*>(pred), static_cast<const u32*>(targ), op->cfg.training, op->loss_image, acc, acc_rows, acc_dirty);
}
int wdgs_tiled_backward_compute_loss_only(wdgs_tiled_backward* op, const void* pred, const void* targ) {
    WDGS_REQUIRE(op && pred && targ, WDGS_E_INVALID, "wdgs_tiled_backward_compute_loss_only: null argument");
    return backward_loss(op, pred, targ, nullptr, 0u, nullptr);
}
static int backward_encode_raster(wdgs_tiled_backward* op, const void* pred, const void* targ, const wdgs_tiled_backward_resources* res) {
    wdgs_device* d = op->dev;
    const u32 w = op->cfg.viewport_width, h = op->cfg.viewport_height, n = op->cfg.num_points;
    // K15 + clearBuffer x4 (tiled-backward-pass.ts:624-627): the clear rides on the loss kernel and is a no-op behind a consuming K17
    if (w > 0 && h > 0) WDGS_TRY(backward_loss(op, pred, targ, op->acc, std::max(n, 1u), op->acc_dirty()));
    else WDGS_TRY(launch_acc_clear_if_dirty(d, op->acc, n, op->acc_dirty()));
    // long tile lists (longlist.h): when the range table is one a forward pass of this device built, that pass's lists serve the backward walk too
    const LongWork* lw = nullptr;
    auto owner = d->range_tables.find(res->tile_offsets_buffer);
    if (owner != d->range_tables.end() && owner->second->ranges_valid && owner->second->long_lists.hdr) lw = &owner->second->long_lists;
    return launch_backward_rasterize(d, op->settings, ceil_div(w, 16), ceil_div(h, 16), static_cast<const u32*>(res->tile_offsets_buffer),
                                     static_cast<const u32*>(res->tile_indices_buffer), static_cast<const u32*>(res->splat_buffer), static_cast<const float*>(res->alpha_texture),
                                     static_cast<const u32*>(res->n_contrib_texture), op->loss_image, op->acc, op->acc_dirty(), lw);
}
int wdgs_tiled_backward_encode(wdgs_tiled_backward* op, const void* pred, const void* targ, const wdgs_tiled_backward_resources* res,
                               const void* gaussians) {
    WDGS_REQUIRE(op && pred && targ && res && gaussians, WDGS_E_INVALID, "wdgs_tiled_backward_encode: null argument");
    WDGS_REQUIRE(res->splat_buffer && res->tile_offsets_buffer && res->tile_indices_buffer && res->camera_buffer && res->alpha_texture && res->n_contrib_texture,
                 WDGS_E_INVALID, "wdgs_tiled_backward_encode: incomplete resources");
    WDGS_TRY(backward_encode_raster(op, pred, targ, res));
    return launch_geometry_backward(op->dev, op->cfg.num_points, static_cast<const float*>(res->camera_buffer), op->settings, static_cast<const u32*>(gaussians), op->acc,
                                    op->gradients);
}
// The two halves of wdgs_tiled_backward_encode, for a batched step: K15 + clear + K16 may run (and be recorded) on any lane at any
// time; K17 of view k also adds the view's gradient to the step's fp32 block, which has to follow view k-1's K17.
int wdgs_tiled_backward_encode_raster(wdgs_tiled_backward* op, const void* pred, const void* targ, const wdgs_tiled_backward_resources* res) {
    WDGS_REQUIRE(op && pred && targ && res, WDGS_E_INVALID, "wdgs_tiled_backward_encode_raster: null argument");
    WDGS_REQUIRE(res->splat_buffer && res->tile_offsets_buffer && res->tile_indices_buffer && res->alpha_texture && res->n_contrib_texture, WDGS_E_INVALID,
                 "wdgs_tiled_backward_encode_raster: incomplete resources");
    return backward_encode_raster(op, pred, targ, res);
}
int wdgs_tiled_backward_encode_geometry(wdgs_tiled_backward* op, const void* camera, const void* gaussians, const wdgs_view_accumulate* into) {
    WDGS_REQUIRE(op && camera && gaussians, WDGS_E_INVALID, "wdgs_tiled_backward_encode_geometry: null argument");
    const float* const cam = static_cast<const float*>(camera);
    const u32* const g = static_cast<const u32*>(gaussians);
    if (!into) return launch_geometry_backward(op->dev, op->cfg.num_points, cam, op->settings, g, op->acc, op->gradients);
    WDGS_REQUIRE(into->sums && into->visible && into->tile_counts && into->guard && into->overflow_word, WDGS_E_INVALID,
                 "wdgs_tiled_backward_encode_geometry: incomplete accumulate target");
    return launch_geometry_backward_accumulate(op->dev, op->cfg.num_points, cam, op->settings, g, op->acc, op->acc_dirty(), op->gradients, static_cast<float*>(into->sums),
                                               static_cast<u32*>(into->visible), static_cast<const u32*>(into->tile_counts), static_cast<u32*>(into->guard),
                                               static_cast<const u32*>(into->overflow_word), into->first ? 1u : 2u);
}
// ---- view-batched K17 (include/webdgs.h)
int wdgs_tiled_backward_encode_geometry_views(wdgs_tiled_backward* const* ops, const void* const* cameras, const void* const* tile_counts, const void* const* overflow_words,
                                              uint32_t count, const void* gaussians, void* sums, void* visible, void* guard, int write_gradients, int continues) {
    WDGS_REQUIRE(ops && cameras && tile_counts && overflow_words && gaussians && sums && visible && guard && count > 0 && count <= WDGS_MAX_BATCH_VIEWS, WDGS_E_INVALID,
                 "wdgs_tiled_backward_encode_geometry_views: invalid argument");
    wdgs_tiled_backward* b0 = ops[0];
    WDGS_REQUIRE(b0, WDGS_E_INVALID, "wdgs_tiled_backward_encode_geometry_views: null pass");
    GeometryViews gv{count};
    for (u32 v = 0; v < count; v++) {
        wdgs_tiled_backward* b = ops[v];
        WDGS_REQUIRE(b && cameras[v] && tile_counts[v] && overflow_words[v], WDGS_E_INVALID, "wdgs_tiled_backward_encode_geometry_views: null argument for view %u", v);
        for (u32 u = 0; u < v; u++) WDGS_REQUIRE(ops[u] != b, WDGS_E_INVALID, "wdgs_tiled_backward_encode_geometry_views: pass %u is given twice (every view has accumulators of its own)", v);
        WDGS_REQUIRE(b->dev == b0->dev && b->cfg.num_points == b0->cfg.num_points && std::memcmp(&b->settings, &b0->settings, sizeof(RenderSettings)) == 0, WDGS_E_STATE,
                     "wdgs_tiled_backward_encode_geometry_views: pass %u differs from pass 0 (cloud size, viewport or settings)", v);
        gv.camera[v] = static_cast<const float*>(cameras[v]); gv.acc[v] = b->acc; gv.acc_dirty[v] = b->acc_dirty(); gv.tile_counts[v] = static_cast<const u32*>(tile_counts[v]);
        gv.overflow[v] = static_cast<const u32*>(overflow_words[v]); gv.gradients[v] = write_gradients ? b->gradients.get() : nullptr;
    }
    return launch_geometry_backward_views(b0->dev, b0->cfg.num_points, b0->settings, static_cast<const u32*>(gaussians), gv, static_cast<float*>(sums),
                                          static_cast<u32*>(visible), static_cast<u32*>(guard), continues ? 1u : 0u);
}
int wdgs_tiled_backward_compute_metric_map(wdgs_tiled_backward* op, const void* pred, const void* targ, float threshold) {
    WDGS_REQUIRE(op && pred && targ, WDGS_E_INVALID, "wdgs_tiled_backward_compute_metric_map: null argument");
    return launch_metric_map(op->dev, op->cfg.viewport_width, op->cfg.viewport_height, static_cast<const u32*>(pred), static_cast<const u32*>(targ), 1000000.0f, threshold,
                             op->metric_err, op->metric_minmax, op->metric_minmax + 2, op->metric_flags);
}
int wdgs_tiled_backward_compute_metric_counts(wdgs_tiled_backward* op, const wdgs_tiled_backward_resources* res, uint32_t num_instances, int clear) {
    WDGS_REQUIRE(op && res && res->splat_buffer && res->tile_offsets_buffer && res->tile_indices_buffer && res->n_contrib_texture, WDGS_E_INVALID,
                 "wdgs_tiled_backward_compute_metric_counts: incomplete resources");
    const u32 n = op->cfg.num_points;
    u32* const counts = op->metric_counts_into ? op->metric_counts_into : op->metric_counts;
    if (clear) WDGS_CHECK_HIP(hipMemsetAsync(counts, 0, (size_t)std::max(n, 1u) * 4, op->dev->stream));
    return launch_metric_count(op->dev, op->settings, ceil_div(op->cfg.viewport_width, 16), ceil_div(op->cfg.viewport_height, 16),
                               static_cast<const u32*>(res->tile_offsets_buffer), static_cast<const u32*>(res->tile_indices_buffer), num_instances,
                               static_cast<const u32*>(res->splat_buffer), n, op->metric_flags, static_cast<const u32*>(res->n_contrib_texture), counts, n);
}
int wdgs_tiled_backward_normalize_metric_counts(wdgs_tiled_backward* op, uint32_t divisor) {
    WDGS_REQUIRE(op, WDGS_E_INVALID, "null op");
    return launch_metric_normalize(op->dev, op->cfg.num_points, divisor, op->metric_counts);
}
int wdgs_tiled_backward_set_viewport(wdgs_tiled_backward* op, uint32_t w, uint32_t h) {
    WDGS_REQUIRE(op && w > 0 && h > 0, WDGS_E_INVALID, "wdgs_tiled_backward_set_viewport: invalid argument");
    op->cfg.viewport_width = w;
    op->cfg.viewport_height = h;
    op->settings.viewport_x = (float)w;
    op->settings.viewport_y = (float)h;
    return backward_alloc_images(op, w, h);
}
int wdgs_tiled_backward_set_training_config(wdgs_tiled_backward* op, const wdgs_training_config* cfg) {
    WDGS_REQUIRE(op && cfg, WDGS_E_INVALID, "null argument");
    op->cfg.training = *cfg;
    if (op->cfg.training.c1 == 0.f) op->cfg.training.c1 = 0.01f * 0.01f;
    if (op->cfg.training.c2 == 0.f) op->cfg.training.c2 = 0.03f * 0.03f;
    return WDGS_OK;
}
int wdgs_tiled_backward_set_dssim_mode(wdgs_tiled_backward* op, uint32_t mode) {
    WDGS_REQUIRE(op, WDGS_E_INVALID, "wdgs_tiled_backward_set_dssim_mode: null op");
    WDGS_REQUIRE(mode == WDGS_DSSIM_REFERENCE || mode == WDGS_DSSIM_GAUSSIAN, WDGS_E_INVALID, "wdgs_tiled_backward_set_dssim_mode: unknown mode %u", mode);
    op->dssim_mode = mode;
    return WDGS_OK;
}
int wdgs_tiled_backward_get_dssim_mode(const wdgs_tiled_backward* op, uint32_t* out) {
    WDGS_REQUIRE(op && out, WDGS_E_INVALID, "wdgs_tiled_backward_get_dssim_mode: null argument");
    *out = op->dssim_mode;
    return WDGS_OK;
}
void* wdgs_tiled_backward_gradients(wdgs_tiled_backward* op) { return op ? op->gradients : nullptr; }
void* wdgs_tiled_backward_metric_counts(wdgs_tiled_backward* op) { return op ? op->metric_counts : nullptr; }
int wdgs_tiled_backward_set_metric_counts_target(wdgs_tiled_backward* op, void* counts_dev) {
    WDGS_REQUIRE(op, WDGS_E_INVALID, "wdgs_tiled_backward_set_metric_counts_target: null op");
    op->metric_counts_into = static_cast<u32*>(counts_dev);
    return WDGS_OK;
}
void* wdgs_tiled_backward_loss_image(wdgs_tiled_backward* op) { return op ? op->loss_image : nullptr; }
void* wdgs_tiled_backward_metric_map(wdgs_tiled_backward* op) { return op ? op->metric_flags : nullptr; }
void* wdgs_tiled_backward_accumulators(wdgs_tiled_backward* op) { return op ? op->acc : nullptr; }
void* wdgs_tiled_backward_metric_minmax(wdgs_tiled_backward* op) { return op ? op->metric_minmax : nullptr; }

int wdgs_downsample_rgba8(wdgs_device* d, const void* src, uint32_t sw, uint32_t sh, void* dst, uint32_t dw, uint32_t dh) {
    WDGS_REQUIRE(d && src && dst && sw && sh && dw && dh, WDGS_E_INVALID, "wdgs_downsample_rgba8: invalid argument");
    return launch_downsample(d, static_cast<const u32*>(src), sw, sh, static_cast<u32*>(dst), dw, dh);
}

// ---------------------------------------------------------------- Optimizer
int wdgs_optimizer_state_sizes(uint32_t n, size_t sizes[6]) {
    WDGS_REQUIRE(sizes, WDGS_E_INVALID, "null argument");
    const size_t N = std::max(n, 1u);  // allocateOptimizerStateBuffers: Math.max(1, ...) (optimizer.ts:28)
    sizes[0] = sizes[1] = sizes[2] = N * 48;
    sizes[3] = N * 12;
    sizes[4] = N * 48 * 4;
    sizes[5] = N * 48 * 2 * 4;
    return WDGS_OK;
}

int wdgs_optimizer_create(wdgs_device* d, uint32_t n, const wdgs_adam_hyperparameters* params, const void* gaussians, const void* sh,
                          const wdgs_optimizer_state* initial, int owns_state, uint32_t initial_iteration, wdgs_optimizer** out) {
    WDGS_REQUIRE(d && out, WDGS_E_INVALID, "wdgs_optimizer_create: null argument");
    auto op = std::make_unique<wdgs_optimizer>();
    op->dev = d;
    op->num_points = n;
    if (params) op->params = *params;
    size_t sz[6];
    wdgs_optimizer_state_sizes(n, sz);
    if (initial) {
        WDGS_REQUIRE(initial->opt_pos && initial->opt_rot && initial->opt_scale && initial->opt_opacity && initial->param_sh && initial->state_sh,
                     WDGS_E_INVALID, "wdgs_optimizer_create: incomplete initial state");
        op->state = *initial;
        void* const given[6] = {initial->opt_pos, initial->opt_rot, initial->opt_scale, initial->opt_opacity, initial->param_sh, initial->state_sh};
        for (int i = 0; owns_state && i < 6; i++) op->owned[i].adopt(static_cast<char*>(given[i]), sz[i]);
        op->iteration = initial_iteration;
    } else {
        WDGS_REQUIRE(gaussians && sh, WDGS_E_INVALID, "wdgs_optimizer_create: point cloud required when no initial state is given");
        for (int i = 0; i < 6; i++) WDGS_TRY(op->owned[i].alloc(sz[i], true, d->stream));
        op->state = wdgs_optimizer_state{op->owned[0].get(), op->owned[1].get(), op->owned[2].get(), op->owned[3].get(), op->owned[4].get(), op->owned[5].get()};
        WDGS_TRY(launch_unpack(d, n, static_cast<const u32*>(gaussians), static_cast<const u32*>(sh), op->state));
    }
    WDGS_TRY(op->dc.alloc(CS_PLANES * (size_t)wdgs_optimizer::cs_pitch(n), true, d->stream));
    WDGS_TRY(launch_cs_load(d, n, op->state, op->cs()));
    *out = op.release();
    return WDGS_OK;
}
int wdgs_optimizer_destroy(wdgs_optimizer* op) {
    if (!op) return WDGS_OK;
    const bool live = wdgs_device_alive(op->dev) && !op->dev->capturing;
    if (!op->owns_state() && live) (void)optimizer_flush_dc(op);  // adopted buffers outlive the optimizer: leave them current
    sync_if_alive(op->dev);
    delete op;
    return WDGS_OK;
}
int wdgs_optimizer_init_from_point_cloud(wdgs_optimizer* op, const void* gaussians, const void* sh) {
    WDGS_REQUIRE(op && gaussians && sh, WDGS_E_INVALID, "wdgs_optimizer_init_from_point_cloud: null argument");
    WDGS_TRY(launch_unpack(op->dev, op->num_points, static_cast<const u32*>(gaussians), static_cast<const u32*>(sh), op->state));
    op->dc_dirty = false;
    return launch_cs_load(op->dev, op->num_points, op->state, op->cs());
}
int wdgs_optimizer_step(wdgs_optimizer* op, void* gaussians, void* sh, const void* gradients, const void* tile_counts) {
    WDGS_REQUIRE(op && gaussians && sh && gradients && tile_counts, WDGS_E_INVALID, "wdgs_optimizer_step: null argument");
    op->iteration++;  // optimizer.ts:301
    op->dc_dirty = true;
    if (op->deferred_sh) op->sh_stale = true;
    return launch_adam_repack(op->dev, op->num_points, op->params, static_cast<const u32*>(tile_counts), static_cast<const u32*>(gradients), op->state, op->cs(),
                              static_cast<u32*>(gaussians), static_cast<u32*>(sh), op->guard, op->deferred_sh ? op->dc_words : nullptr);
}
// K17 + K18 + K19 in one pass over the Gaussians (the single-view step): `bwd` must have run wdgs_tiled_backward_encode_raster for this view.
int wdgs_optimizer_step_with_geometry(wdgs_optimizer* op, wdgs_tiled_backward* bwd, const void* camera, void* gaussians, void* sh, const void* tile_counts) {
    WDGS_REQUIRE(op && bwd && camera && gaussians && sh && tile_counts, WDGS_E_INVALID, "wdgs_optimizer_step_with_geometry: null argument");
    WDGS_REQUIRE(bwd->cfg.num_points == op->num_points, WDGS_E_STATE, "wdgs_optimizer_step_with_geometry: the backward pass holds %u Gaussians, the optimizer %u",
                 bwd->cfg.num_points, op->num_points);
    op->iteration++;  // optimizer.ts:301
    op->dc_dirty = true;
    if (op->deferred_sh) op->sh_stale = true;
    return launch_geometry_backward_adam(op->dev, op->num_points, static_cast<const float*>(camera), bwd->settings, static_cast<u32*>(gaussians), bwd->acc, bwd->acc_dirty(),
                                         bwd->gradient_output ? bwd->gradients : nullptr, op->params, static_cast<const u32*>(tile_counts), op->state, op->cs(),
                                         static_cast<u32*>(sh), op->guard, op->deferred_sh ? op->dc_words : nullptr);
}
int wdgs_optimizer_step_f32(wdgs_optimizer* op, void* gaussians, void* sh, const void* grad_f32, const void* visible) {
    WDGS_REQUIRE(op && gaussians && sh && grad_f32 && visible, WDGS_E_INVALID, "wdgs_optimizer_step_f32: null argument");
    op->iteration++;
    op->dc_dirty = true;
    if (op->deferred_sh) op->sh_stale = true;
    return launch_adam_repack_f32(op->dev, 0, op->num_points, op->params, static_cast<const u32*>(visible), static_cast<const float*>(grad_f32), op->state, op->cs(),
                                  static_cast<u32*>(gaussians), static_cast<u32*>(sh), op->guard, op->dev->host_guard, nullptr, op->deferred_sh ? op->dc_words : nullptr);
}
int wdgs_optimizer_step_f32_range(wdgs_optimizer* op, void* gaussians, void* sh, const void* grad_f32, const void* visible, uint32_t first, uint32_t count,
                                  void* rows_out) {
    WDGS_REQUIRE(op && gaussians && sh && grad_f32 && visible, WDGS_E_INVALID, "wdgs_optimizer_step_f32_range: null argument");
    WDGS_REQUIRE((uint64_t)first + count <= op->num_points, WDGS_E_INVALID, "wdgs_optimizer_step_f32_range: [%u, %u) exceeds %u points", first, first + count,
                 op->num_points);
    op->iteration++;
    op->dc_dirty = true;
    if (op->deferred_sh) op->sh_stale = true;
    return launch_adam_repack_f32(op->dev, first, count, op->params, static_cast<const u32*>(visible), static_cast<const float*>(grad_f32), op->state, op->cs(),
                                  static_cast<u32*>(gaussians), static_cast<u32*>(sh), op->guard, op->dev->host_guard, static_cast<u32*>(rows_out),
                                  op->deferred_sh ? op->dc_words : nullptr);
}
int wdgs_optimizer_set_guard(wdgs_optimizer* op, const void* flag) {
    WDGS_REQUIRE(op, WDGS_E_INVALID, "null op");
    op->guard = static_cast<const u32*>(flag);
    return WDGS_OK;
}
int wdgs_optimizer_state_changed(wdgs_optimizer* op) {
    WDGS_REQUIRE(op, WDGS_E_INVALID, "null op");
    op->dc_dirty = false;
    return launch_cs_load(op->dev, op->num_points, op->state, op->cs());
}
int wdgs_apply_repacked_rows(wdgs_device* d, uint32_t n, const void* rows, uint32_t skip_first, uint32_t skip_count, const void* guard, void* gaussians,
                             void* sh) {
    WDGS_REQUIRE(d && rows && gaussians && sh, WDGS_E_INVALID, "wdgs_apply_repacked_rows: null argument");
    return launch_apply_rows(d, n, static_cast<const u32*>(rows), skip_first, skip_count, static_cast<const u32*>(guard), d->host_guard, static_cast<u32*>(gaussians),
                             static_cast<u32*>(sh), nullptr);
}
// The same for a replica whose optimizer defers its SH writes: the gathered DC halves go to its compact words as well.
int wdgs_optimizer_apply_repacked_rows(wdgs_optimizer* op, const void* rows, uint32_t skip_first, uint32_t skip_count, const void* guard, void* gaussians, void* sh) {
    WDGS_REQUIRE(op && rows && gaussians && sh, WDGS_E_INVALID, "wdgs_optimizer_apply_repacked_rows: null argument");
    if (op->deferred_sh) op->sh_stale = true;
    return launch_apply_rows(op->dev, op->num_points, static_cast<const u32*>(rows), skip_first, skip_count, static_cast<const u32*>(guard), op->dev->host_guard,
                             static_cast<u32*>(gaussians), static_cast<u32*>(sh), op->deferred_sh ? op->dc_words : nullptr);
}
// ---- deferred SH writes (no reference counterpart)
int wdgs_optimizer_set_deferred_sh(wdgs_optimizer* op, void* sh, int enabled) {
    WDGS_REQUIRE(op && sh, WDGS_E_INVALID, "wdgs_optimizer_set_deferred_sh: null argument");
    WDGS_REQUIRE(!op->dev->capturing, WDGS_E_STATE, "wdgs_optimizer_set_deferred_sh while recording a command buffer");
    if (!enabled) {
        if (op->deferred_sh && op->sh_stale) WDGS_TRY(launch_dc_words_flush(op->dev, op->num_points, op->dc_words, static_cast<u32*>(sh)));
        op->deferred_sh = false;
        op->sh_stale = false;
        return WDGS_OK;
    }
    if (!op->dc_words) WDGS_TRY(op->dc_words.alloc((size_t)2 * std::max(op->num_points, 1u), true, op->dev->stream));
    if (!op->deferred_sh || !op->sh_stale) WDGS_TRY(launch_dc_words_load(op->dev, op->num_points, static_cast<const u32*>(sh), op->dc_words));  // the rows are current: take their DC halves
    op->deferred_sh = true;
    return WDGS_OK;
}
void* wdgs_optimizer_dc_words(wdgs_optimizer* op) { return (op && op->deferred_sh) ? op->dc_words : nullptr; }
int wdgs_optimizer_flush_sh(wdgs_optimizer* op, void* sh) {
    WDGS_REQUIRE(op && sh, WDGS_E_INVALID, "wdgs_optimizer_flush_sh: null argument");
    if (!op->deferred_sh || !op->sh_stale) return WDGS_OK;
    WDGS_REQUIRE(!op->dev->capturing, WDGS_E_STATE, "wdgs_optimizer_flush_sh while recording a command buffer");
    WDGS_TRY(launch_dc_words_flush(op->dev, op->num_points, op->dc_words, static_cast<u32*>(sh)));  // stream-ordered: later kernels and copies on this device see current rows
    op->sh_stale = false;
    return WDGS_OK;
}
int wdgs_tiled_forward_set_dc_source(wdgs_tiled_forward* op, const void* dc_words) {
    WDGS_REQUIRE(op, WDGS_E_INVALID, "wdgs_tiled_forward_set_dc_source: null op");
    op->dc_source = static_cast<const u32*>(dc_words);
    return WDGS_OK;
}
int wdgs_guard_accumulate(wdgs_device* d, void* flag, const void* src, int overwrite) {
    WDGS_REQUIRE(d && flag && src, WDGS_E_INVALID, "wdgs_guard_accumulate: null argument");
    return launch_guard_accumulate(d, static_cast<u32*>(flag), static_cast<const u32*>(src), overwrite ? 1u : 0u);
}
int wdgs_accumulate_gradients(wdgs_device* d, uint32_t n, const void* gradients, const void* tile_counts, void* acc, void* visible) {
    WDGS_REQUIRE(d && gradients && tile_counts && acc && visible, WDGS_E_INVALID, "wdgs_accumulate_gradients: null argument");
    return launch_accumulate_gradients(d, n, static_cast<const u32*>(gradients), static_cast<const u32*>(tile_counts), static_cast<float*>(acc), static_cast<u32*>(visible));
}
int wdgs_store_gradients(wdgs_device* d, uint32_t n, const void* gradients, const void* tile_counts, void* acc, void* visible) {
    WDGS_REQUIRE(d && gradients && tile_counts && acc && visible, WDGS_E_INVALID, "wdgs_store_gradients: null argument");
    return launch_store_gradients(d, n, static_cast<const u32*>(gradients), static_cast<const u32*>(tile_counts), static_cast<float*>(acc), static_cast<u32*>(visible));
}
uint32_t wdgs_optimizer_get_iteration(const wdgs_optimizer* op) { return op ? op->iteration : 0; }
int wdgs_optimizer_advance_iteration(wdgs_optimizer* op, uint32_t count) {
    WDGS_REQUIRE(op, WDGS_E_INVALID, "null op");
    op->iteration += count;
    if (count) op->dc_dirty = true;  // a recorded step() was re-submitted
    if (count && op->deferred_sh) op->sh_stale = true;
    return WDGS_OK;
}
int wdgs_optimizer_get_hyperparameters(const wdgs_optimizer* op, wdgs_adam_hyperparameters* out) {
    WDGS_REQUIRE(op && out, WDGS_E_INVALID, "null argument");
    *out = op->params;
    return WDGS_OK;
}
int wdgs_optimizer_set_hyperparameters(wdgs_optimizer* op, const wdgs_adam_hyperparameters* p) {
    WDGS_REQUIRE(op && p, WDGS_E_INVALID, "null argument");
    op->params = *p;
    return WDGS_OK;
}
int wdgs_optimizer_get_state(wdgs_optimizer* op, wdgs_optimizer_state* out) {
    WDGS_REQUIRE(op && out, WDGS_E_INVALID, "null argument");
    WDGS_TRY(optimizer_flush_dc(op));  // stream-ordered: later kernels and copies on this device see current SH rows
    *out = op->state;
    return WDGS_OK;
}
int wdgs_optimizer_release_state(wdgs_optimizer* op, wdgs_optimizer_state* out) {
    WDGS_REQUIRE(op && out, WDGS_E_INVALID, "null argument");
    WDGS_TRY(optimizer_flush_dc(op));
    *out = op->state;
    for (auto& m : op->owned) (void)m.release();   // the arrays are the caller's from here on: `state` stays the view of them
    return WDGS_OK;
}

}  // extern "C"
