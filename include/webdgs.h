/*
 * webdgs.h -- C ABI of libwebdgs_hip.so: the MI355X (gfx950) hot path of krispy-kenay/WebDGS.
 *
 * The reference has no FFI: its boundary is the set of TypeScript operator classes that
 * src/trainer.ts and src/viewer.ts construct.  Every entry point below names the
 * reference interface it replaces (paths relative to the reference's src/).  Conventions:
 *
 *   - every function returns int: 0 = WDGS_OK, <0 = WDGS_E_*; wdgs_last_error() gives the text
 *     (the reference throws `Error`, e.g. renderers/tiled-rasterizer.ts:308-330);
 *   - `void*` arguments named *_dev are DEVICE pointers (hipMalloc / torch / wdgs_buffer_ptr); no torch or
 *     HIP types appear in signatures;
 *   - ops own the buffers they create and free them in *_destroy (idempotent on NULL), as the reference's
 *     destroy() methods do (renderers/tiled-forward-pass.ts:518-533); borrowed pointers are never freed;
 *   - "encode" = the reference's encode(encoder, ...): work is queued on the device's HIP stream in call
 *     order and runs asynchronously; wdgs_device_synchronize() = queue.onSubmittedWorkDone()
 *     (trainer.ts:639-645).  wdgs_buffer_write() is stream-ordered (queue.writeBuffer, camera/camera.ts:194);
 *   - sizes that the reference derives on the GPU (total tile entries) stay on the GPU: no host read-back
 *     inside a step.  Capacity overflow is a hard error reported by *_check / wdgs_device_synchronize
 *     (the reference silently overruns: SURVEY Q1, Q2);
 *   - handles are not thread-safe; use one host thread per wdgs_device;
 *   - teardown order: destroy command buffers and ops, then wdgs_comm, then the device.  An op destroyed AFTER its device
 *     (a host finalising objects in arbitrary order at exit) only releases its memory and never touches the dead device;
 *     wdgs_device_destroy is idempotent.
 *
 * Data layouts (byte-exact with the reference unless marked INTERNAL):
 *   Gaussian        6 x u32 = 12 fp16: x y z opacity_raw | rot w x y z | log-sigma x y z, pad   shaders/common.wgsl:20-24
 *   SH              24 x u32 = 48 fp16, [k][rgb], 16 coefficient slots                          shaders/tiled-forward.wgsl:64-86
 *   Splat           6 x u32 fp16 pairs: ndc.xy | extent.xy px | conic.xy | conic.z,0 | r,g | b,opacity   shaders/common.wgsl:26-33
 *   CameraUniforms  68 f32: view, view_inv, proj, proj_inv (column-major), viewport.xy, focal.xy  shaders/common.wgsl:1-8
 *   GaussianGradient 8 x u32 = 16 fp16: dpos.xyz dopacity | drot.wxyz | dlogsigma.xyz 0 | drgb 0  shaders/tiled-backward.wgsl:18-23
 *   OptVec4 {param,m,v: vec4f} 48 B; OptFloat {param,m,v} 12 B; param_sh 48 f32; state_sh 48 x (m,v)   renderers/optimizer.ts:7-11
 *   images          rgba8unorm, row-major, W*H*4 bytes (textures in the reference)
 *   grad accumulators INTERNAL: i32 x 12 per Gaussian {mean.x, mean.y, conic.x, conic.y, conic.z, opacity, r, g, b as four partial sums}
 *                   (the reference keeps four arrays, renderers/tiled-backward-pass.ts:249-252; same fixed-point x1e6 values)
 */
#ifndef WEBDGS_H
#define WEBDGS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WDGS_OK 0
#define WDGS_E_INVALID (-1)  /* bad argument / API misuse */
#define WDGS_E_HIP (-2)      /* HIP runtime error */
#define WDGS_E_CAPACITY (-3) /* a device-side capacity was exceeded (tile entries, densify output) */
#define WDGS_E_STATE (-4)    /* getter before first encode, mismatched sizes, ... */

typedef struct wdgs_device wdgs_device;
typedef struct wdgs_buffer wdgs_buffer;
typedef struct wdgs_prefix_scanner wdgs_prefix_scanner;
typedef struct wdgs_sorter wdgs_sorter;
typedef struct wdgs_tiled_forward wdgs_tiled_forward;
typedef struct wdgs_tiled_rasterizer wdgs_tiled_rasterizer;
typedef struct wdgs_tiled_backward wdgs_tiled_backward;
typedef struct wdgs_optimizer wdgs_optimizer;
typedef struct wdgs_densify_prune wdgs_densify_prune;
typedef struct wdgs_command_buffer wdgs_command_buffer;

const char* wdgs_last_error(void);
/* ABI version of this header; bumped on any signature change. */
int wdgs_abi_version(void);

/* ---------------------------------------------------------------- device / queue
 * Replaces GPUDevice + GPUQueue (main.ts:186-201).  external_hip_stream may be NULL (the device creates its own
 * stream) or a hipStream_t the caller owns (e.g. torch.cuda.current_stream().cuda_stream). */
int wdgs_device_create(int hip_ordinal, void* external_hip_stream, wdgs_device** out);
int wdgs_device_destroy(wdgs_device* dev);
/* queue.onSubmittedWorkDone(): waits for the stream, then reports deferred device-side errors. */
int wdgs_device_synchronize(wdgs_device* dev);
/* device.limits (trainer.ts:147 reads maxStorageBufferBindingSize to bound the densify rebuild): the device's memory in bytes.  free_bytes counts what
 * the library's allocation cache holds (cached_bytes: freed blocks kept for the next allocation of their size class) as used.  Any pointer may be NULL. */
int wdgs_device_memory_info(wdgs_device* dev, size_t* free_bytes, size_t* total_bytes, size_t* cached_bytes);
/* Per-kernel hipEvent timing (the reference only has a wall-clock meter, trainer.ts:570,647-651). */
int wdgs_device_set_profiling(wdgs_device* dev, int enabled);
/* After a synchronize: copies up to `cap` records; returns the number of distinct kernels through *count. */
typedef struct wdgs_kernel_time {
    char name[48];
    uint32_t launches;
    float total_ms;
} wdgs_kernel_time;
int wdgs_device_get_kernel_times(wdgs_device* dev, wdgs_kernel_time* out, uint32_t cap, uint32_t* count);
int wdgs_device_reset_kernel_times(wdgs_device* dev);
/* Lanes.  A device has WDGS_MAX_LANES in-order queues: lane 0 is its stream (the one given to wdgs_device_create), the others are
 * internal and created on first use.  wdgs_device_select_lane makes `lane` the target of every later encode / submit / copy; work
 * on different lanes may run concurrently and is ordered only where wdgs_device_lane_order says so: everything submitted to lane
 * `waiter` after the call runs after everything submitted to lane `signal` before it (an event, no host wait).
 * wdgs_device_synchronize waits for all of them.  The reference has one GPUQueue and no counterpart; a batched step
 * (views_per_rank > 1, BASELINE config c4) uses the lanes to run the bandwidth-bound stages of one view beside the rasterization
 * kernels of another.  Each lane needs its own forward / rasterizer / backward ops (their intermediate buffers are per op); the
 * point cloud is shared read-only until the lanes are joined in front of the optimizer step.  Neither call is allowed while
 * recording. */
#define WDGS_MAX_LANES 4
#define WDGS_MAX_BATCH_VIEWS 16 /* views one view-batched K1 / K17 launch covers (wdgs_tiled_forward_project_views) */
int wdgs_device_select_lane(wdgs_device* dev, int lane);
int wdgs_device_lane_order(wdgs_device* dev, int waiter_lane, int signal_lane);
/* A position on `lane`, remembered in one of WDGS_MAX_BATCH_VIEWS numbered marks, for other lanes to wait for later
 * (wdgs_device_lane_order records and waits in one call). */
int wdgs_device_lane_mark(wdgs_device* dev, int lane, int mark);
int wdgs_device_lane_wait_mark(wdgs_device* dev, int lane, int mark);

/* ---------------------------------------------------------------- recorded command buffers (hipGraph)
 * Replaces device.createCommandEncoder() ... encoder.finish() -> GPUCommandBuffer -> queue.submit([cmd]) (trainer.ts:603-645).
 * Between begin and end every encode call is captured into a HIP graph instead of running; wdgs_queue_submit replays it on
 * the device's stream.  Unlike a GPUCommandBuffer the result may be submitted any number of times, as long as the buffers it
 * was recorded against are alive (all sizes the kernels need are read on the device, so a replay adapts to new data).
 * Calls that synchronise or allocate (copy_to_host, *_check, first-use allocations inside encode) are not allowed while
 * recording: run one eager step first.  Per-kernel profiling is suspended inside a recording. */
int wdgs_encoder_begin(wdgs_device* dev);
int wdgs_encoder_finish(wdgs_device* dev, wdgs_command_buffer** out);
/* Drops an open recording (an encode between begin and finish failed, or the host threw): ends the capture, discards the partial
 * graph and returns the device to eager mode.  A no-op when nothing is being recorded, so error paths may call it unconditionally.
 * The reference has no counterpart: an encoder that is never finished is simply garbage-collected. */
int wdgs_encoder_abort(wdgs_device* dev);
int wdgs_queue_submit(wdgs_device* dev, wdgs_command_buffer* cmd);
int wdgs_command_buffer_destroy(wdgs_command_buffer* cmd);
/* queue.onSubmittedWorkDone() as a completion callback (trainer.ts:639-645): `fn(user)` runs on a runtime thread once everything
 * submitted to the device's stream before this call has finished.  It must not call back into this library or HIP; an N-API
 * host resolves its Promise from it through a thread-safe function.  Deferred device-side checks (tile-entry overflow) are
 * still reported by wdgs_device_synchronize / wdgs_tiled_forward_check. */
typedef void (*wdgs_done_callback)(void* user);
int wdgs_queue_on_done(wdgs_device* dev, wdgs_done_callback fn, void* user);
/* The same promise, kept and awaited later: wdgs_queue_mark returns a ticket for "everything submitted to the current lane so far",
 * wdgs_queue_wait blocks the host until that work has finished and then reports the deferred device-side errors exactly as
 * wdgs_device_synchronize does.  A host that waits for step k-1's ticket after submitting step k (`const p = queue.onSubmittedWorkDone();
 * ...; await previous`) keeps the device busy across the step boundary; trainer.ts:639-645 awaits at once, which is mark + wait.
 * At most WDGS_TICKET_RING tickets stay distinct: an older one waits for the mark that took its slot (later in the same queue). */
#define WDGS_TICKET_RING 8
int wdgs_queue_mark(wdgs_device* dev, uint64_t* ticket);
int wdgs_queue_wait(wdgs_device* dev, uint64_t ticket);

/* Raw device<->host copies on the device's stream (copy_to_host synchronises): mapAsync/getMappedRange
 * (trainer.ts:455-458) and queue.writeBuffer. */
int wdgs_copy_to_host(wdgs_device* dev, void* dst_host, const void* src_dev, size_t bytes);
int wdgs_copy_to_device(wdgs_device* dev, void* dst_dev, const void* src_host, size_t bytes);
int wdgs_memset(wdgs_device* dev, void* dst_dev, int value, size_t bytes); /* encoder.clearBuffer */
/* encoder.copyBufferToBuffer(src, srcOffset, dst, dstOffset, size) (the staging copy of trainer.ts:445): device to device on the
 * current lane, stream-ordered; recordable.  The ranges must not overlap. */
int wdgs_copy_buffer_to_buffer(wdgs_device* dev, void* dst_dev, const void* src_dev, size_t bytes);

/* ---------------------------------------------------------------- buffers (for hosts without their own allocator)
 * Replaces device.createBuffer / GPUBuffer.destroy; contents are zero-filled like WebGPU buffers. */
int wdgs_buffer_create(wdgs_device* dev, size_t bytes, wdgs_buffer** out);
int wdgs_buffer_destroy(wdgs_buffer* buf);
void* wdgs_buffer_ptr(const wdgs_buffer* buf);
size_t wdgs_buffer_size(const wdgs_buffer* buf);
int wdgs_buffer_write(wdgs_device* dev, wdgs_buffer* buf, size_t offset, const void* src_host, size_t bytes);
int wdgs_buffer_read(wdgs_device* dev, const wdgs_buffer* buf, size_t offset, void* dst_host, size_t bytes);
/* mapAsync(READ) counterpart (trainer.ts:455-458): queues the copy on the device's stream and returns; dst_host is valid after
 * a later wdgs_queue_on_done callback or wdgs_device_synchronize.  dst_host should come from wdgs_host_alloc (pinned) for the
 * copy to overlap with the host. */
int wdgs_buffer_read_async(wdgs_device* dev, const wdgs_buffer* buf, size_t offset, void* dst_host, size_t bytes);
int wdgs_host_alloc(size_t bytes, void** out_host); /* pinned host memory */
int wdgs_host_free(void* host);

/* ---------------------------------------------------------------- prefix scanner
 * Replaces get_prefix_scanner(maxElements, device): PrefixScanner (prefix/prefix.ts:140, interface 26-43).
 * Exclusive u32 scan.  No 2 097 152-element cap. */
int wdgs_prefix_scanner_create(wdgs_device* dev, uint32_t max_elements, wdgs_prefix_scanner** out);
int wdgs_prefix_scanner_destroy(wdgs_prefix_scanner* s);
void* wdgs_prefix_scanner_input(wdgs_prefix_scanner* s);  /* input_buffer  (u32[max_elements]) */
void* wdgs_prefix_scanner_output(wdgs_prefix_scanner* s); /* output_buffer (u32[max_elements]) */
int wdgs_prefix_scanner_set_count(wdgs_prefix_scanner* s, uint32_t count);
int wdgs_prefix_scanner_scan(wdgs_prefix_scanner* s);
/* Scan arbitrary device arrays with this scanner's scratch (count <= max_elements). */
int wdgs_prefix_scanner_scan_ptr(wdgs_prefix_scanner* s, const void* in_dev, void* out_dev, uint32_t count);

/* ---------------------------------------------------------------- dynamic sorter
 * Replaces get_dynamic_sorter(maxCapacity, device, statsBuffer): DynamicSortStuff (sort/sort_dynamic.ts:252,
 * interface 9-24).  Stable ascending LSD radix sort of (key u32, value u32) pairs; the element count is read on
 * the device from stats_dev[0] (TilePipelineStats.total_tile_entries).  Results land in
 * ping_pong[final_out_index] (sort_dynamic.ts:24, 386).  key_bits limits the passes to the significant digits
 * (the reference always runs 4). */
int wdgs_sorter_create(wdgs_device* dev, uint32_t max_capacity, const void* stats_dev, wdgs_sorter** out);
int wdgs_sorter_destroy(wdgs_sorter* s);
void* wdgs_sorter_keys(wdgs_sorter* s, int ping_pong_index);   /* sort_depths_buffer  */
void* wdgs_sorter_values(wdgs_sorter* s, int ping_pong_index); /* sort_indices_buffer */
int wdgs_sorter_sort(wdgs_sorter* s, uint32_t key_bits);
int wdgs_sorter_final_out_index(wdgs_sorter* s);  /* DynamicSortStuff.final_out_index */
uint32_t wdgs_sorter_capacity(wdgs_sorter* s);

/* ---------------------------------------------------------------- TiledForwardPass
 * Replaces `new TiledForwardPass(device, pointCloud, cameraBuffer, config)` (renderers/tiled-forward-pass.ts:120-125,
 * config 24-31), .encode (341-387), setters (389-425), .getResources (428-443), getters (445-459), .destroy (518). */
typedef struct wdgs_tiled_forward_config {
    uint32_t num_points;         /* pointCloud.num_points */
    uint32_t sh_deg;             /* pointCloud.sh_deg */
    uint32_t viewport_width;
    uint32_t viewport_height;
    float gaussian_scale;        /* default 1.0 (declared, unused by the tiled path: SURVEY A3) */
    float point_size_px;         /* default 3.0 */
    float max_splat_radius_px;   /* default 128.0 */
    uint32_t render_mode;        /* 1 = 'gaussian', 0 = 'pointcloud' */
    uint32_t max_tile_entries;   /* 0 = auto: max(30*N, 1<<20) rounded up to 4096 */
    uint32_t compat_caps;        /* 1 = reproduce the reference's capacity caps (min(30N, 32Mi, 2097152) -> x3840) */
} wdgs_tiled_forward_config;

typedef struct wdgs_tiled_forward_resources { /* TiledForwardResources (tiled-forward-pass.ts:33-46) */
    void* splat_buffer;        /* Splat[num_points] */
    void* depths_buffer;       /* u32[num_points] ordered-uint view z */
    void* tile_keys_buffer;    /* u32[max_tile_entries]  (sorted after encode) */
    void* tile_indices_buffer; /* u32[max_tile_entries]  (sorted after encode) */
    void* tile_offsets_buffer; /* u32[num_points] per-GAUSSIAN exclusive scan */
    void* tile_counts_buffer;  /* u32[num_points] */
    void* stats_buffer;        /* u32[4] {total_tile_entries, visible_gaussians, overflow_flag, pad} */
    uint32_t num_tiles_x, num_tiles_y, total_tiles, max_tile_entries;
    float settings[7];         /* RenderSettings (shaders/common.wgsl:10-18) */
} wdgs_tiled_forward_resources;

int wdgs_tiled_forward_create(wdgs_device* dev, const wdgs_tiled_forward_config* cfg, wdgs_tiled_forward** out);
int wdgs_tiled_forward_destroy(wdgs_tiled_forward* op);
/* The point cloud changed size (densify / prune).  applyPointCloudSwap (trainer.ts:201-237) destroys every pass and builds new ones; this
 * keeps the pass: its buffers are reused when large enough and re-allocated with 25 % headroom when not, and the pass is left in the
 * state of a freshly created one for num_points (zeroed per-Gaussian buffers, nothing encoded, max_tile_entries by the creation
 * formula).  Synchronises; not allowed while recording; command buffers recorded against the pass must be dropped by the caller. */
int wdgs_tiled_forward_resize(wdgs_tiled_forward* op, uint32_t num_points);
/* encode(encoder, {skipSort}): K1 project+count, scan, stats, K6 emit, sort. gaussians/sh/camera are device pointers. */
int wdgs_tiled_forward_encode(wdgs_tiled_forward* op, const void* gaussians_dev, const void* sh_dev, const void* camera_dev, int skip_sort);
int wdgs_tiled_forward_set_viewport(wdgs_tiled_forward* op, uint32_t width, uint32_t height);
int wdgs_tiled_forward_set_render_mode(wdgs_tiled_forward* op, uint32_t render_mode);
int wdgs_tiled_forward_set_point_size(wdgs_tiled_forward* op, float point_size_px);
int wdgs_tiled_forward_set_gaussian_scale(wdgs_tiled_forward* op, float scale);
int wdgs_tiled_forward_get_resources(wdgs_tiled_forward* op, wdgs_tiled_forward_resources* out);
/* Synchronises and returns WDGS_E_CAPACITY if the last encode overflowed max_tile_entries; stats_out (4 x u32) optional. */
int wdgs_tiled_forward_check(wdgs_tiled_forward* op, uint32_t* stats_out);
/* Long tile lists.  The reference stages at most 32 x 256 = 8 192 entries of a tile (tiled-rasterizer.wgsl:59-60, 125) and drops the rest; this
 * library composites every entry, and gives the blocks of a tile with more than `threshold` entries per-PIXEL lists, built and walked by tasks that the
 * waves of the rasterization kernels work off themselves (csrc/longlist.h) -- no launch, no host decision: the path is part of every recording and taken
 * on the device.  Results do not depend on it.  A pass is created with threshold 2048, room for 1024 (block, 64-entry chunk) slots and 8192 list rows (13 MB);
 * the path is taken by ALL long tiles of a frame or by none: a frame whose long tiles want more slots than there are is composited the ordinary way
 * (correct; slow if its long tiles are few, right if they are many: a frame full of long tiles keeps the chip busy without it).  set_long_lists re-sizes the work (threshold 0: off; items / rows 0: keep);
 * synchronises, not allowed while recording, command buffers recorded against the pass must be dropped.  long_list_stats (synchronises) returns
 * {block records wanted, item slots wanted, forward queue position, backward queue position, rows handed out, rows wanted, stall code (0 = none), 0,
 *  max_items, max_blocks, max_rows, threshold} of the last frame: a host compares wanted with the capacities and enlarges them -- up to a cap of its
 * choosing (the Trainers: 8 192 slots, 65 536 rows). */
int wdgs_tiled_forward_set_long_lists(wdgs_tiled_forward* op, uint32_t threshold, uint32_t max_items, uint32_t max_rows);
int wdgs_tiled_forward_long_list_stats(wdgs_tiled_forward* op, uint32_t stats_out[12]);

/* ---------------------------------------------------------------- TiledRasterizer
 * Replaces `new TiledRasterizer({device, forwardPass, format})` (renderers/tiled-rasterizer.ts:57), .encode(encoder,w,h)
 * (180-242: tile ranges K12-K13 + composite K14), texture getters (308-330), .destroy (359).  The tile grid follows
 * the forward pass's CURRENT viewport (fixes the stale-grid host bug). */
int wdgs_tiled_rasterizer_create(wdgs_device* dev, wdgs_tiled_forward* forward, uint32_t compat_caps, wdgs_tiled_rasterizer** out);
int wdgs_tiled_rasterizer_destroy(wdgs_tiled_rasterizer* op);
int wdgs_tiled_rasterizer_encode(wdgs_tiled_rasterizer* op, uint32_t width, uint32_t height);
/* Getters fail with WDGS_E_STATE before the first encode, as the reference throws. */
int wdgs_tiled_rasterizer_get_output(wdgs_tiled_rasterizer* op, void** rgba8_dev);        /* getOutputTextureView   */
int wdgs_tiled_rasterizer_get_alpha(wdgs_tiled_rasterizer* op, void** final_t_dev);       /* getAlphaTextureView  f32[W*H] */
int wdgs_tiled_rasterizer_get_n_contrib(wdgs_tiled_rasterizer* op, void** n_contrib_dev); /* getNContribTextureView u32[W*H] */
int wdgs_tiled_rasterizer_get_tile_offsets(wdgs_tiled_rasterizer* op, void** ranges_dev); /* getTileOffsetsBuffer: per-TILE table u32[T+1] */
/* blitToTexture (tiled-rasterizer.ts:333-357, shaders/blit.wgsl vs_main/fs_main): full-target draw that samples the output
 * image with a linear clamp-to-edge sampler into an rgba8 target of any size (the viewer's swap-chain image, viewer.ts:76-86).
 * WDGS_E_STATE before the first encode, as the reference throws. */
int wdgs_tiled_rasterizer_blit(wdgs_tiled_rasterizer* op, void* target_rgba8_dev, uint32_t target_width, uint32_t target_height);

/* Depth images.  The reference renders colour only and has no counterpart to any of the three entries below.
 * encode_depth composites the view-space depths of the frame the last encode rasterized, with the weights w_i = alpha_i (1 - A) the colour was
 * composited with (same records, same order, same arithmetic): WDGS_DEPTH_WEIGHT_SUM is A = sum w_i (1.0f - A is the alpha texture bit for bit),
 * WDGS_DEPTH_EXPECTED is (sum w_i z_i) / A (0 where A is not > 0), WDGS_DEPTH_MEDIAN the z of the first record at which A reaches 0.5 (0 if none).
 * `kinds` is a non-empty set of these bits (WDGS_E_INVALID otherwise); only the images asked for are written, and each is allocated at the first
 * encode_depth that asks for it -- which therefore cannot be recorded (WDGS_E_STATE); later ones can.  WDGS_E_STATE before encode, and when the
 * forward pass is in point-cloud render mode (no weights).  No reference counterpart. */
#define WDGS_DEPTH_EXPECTED   1u
#define WDGS_DEPTH_MEDIAN     2u
#define WDGS_DEPTH_WEIGHT_SUM 4u
int wdgs_tiled_rasterizer_encode_depth(wdgs_tiled_rasterizer* op, uint32_t kinds);
/* f32[W*H] of ONE kind; WDGS_E_STATE if the last encode_depth did not write it.  No reference counterpart. */
int wdgs_tiled_rasterizer_get_depth(wdgs_tiled_rasterizer* op, uint32_t kind, void** f32_dev);
/* A depth image as rgba8 for presentation: t = clamp((1/z - 1/far) / (1/near - 1/far), 0, 1), grey = round(255 t), alpha 255; depth 0 (no weight
 * at the pixel) is black.  Requires 0 < near < far < inf.  Writes width*height pixels of any rgba8 buffer.  No reference counterpart. */
int wdgs_depth_to_rgba8(wdgs_device* dev, const void* depth_f32_dev, uint32_t width, uint32_t height, float near_z, float far_z, void* rgba8_dev);

/* Per-Gaussian render contribution.  No reference counterpart: the reference prunes by opacity alone.
 * Attributes the weights w = alpha (1 - A) of the frame the last encode rasterized -- the active (pixel, record) pairs of section 10, w with the
 * compositing weight's bits -- to their Gaussians.  `stats_dev` holds one 16-byte record per Gaussian of the forward pass, 16-byte aligned:
 *     { uint64 sum_q; uint32 max_bits; uint32 pixels; }
 * sum_q += (uint32)(w * 2^24) (truncating; the weight sum is sum_q * 2^-24), max_bits = max(max_bits, the f32 bits of w), pixels += 1 (modulo 2^32)
 * per active pair; a NaN weight adds to none.  The call ADDS into the buffer, which the caller owns and clears: views accumulate, and the result does
 * not depend on the order of views, waves or launches (integer atomics only).  Nothing is allocated, so the call records into a command buffer.
 * WDGS_E_STATE before encode, and when the forward pass is in point-cloud render mode (no weights); WDGS_E_INVALID on a null or misaligned pointer. */
int wdgs_tiled_rasterizer_encode_contribution(wdgs_tiled_rasterizer* op, void* stats_dev);

/* Normal maps.  The reference renders colour only and has no counterpart to any of the six entries below.
 * encode_normal first gives every Gaussian of `gaussians_dev` one packed view-space normal under `camera_dev` -- the cloud and the 68-float block the
 * forward pass was last encoded with, which the caller names again as in wdgs_tiled_forward_encode.  The normal is the Gaussian's shortest axis
 * (row k of R(q / |q|), k the index of the smallest log-scale, ties to the lowest index), in view space, unit length, turned toward the camera, packed
 * octahedrally into snorm16 x 2; the word 0x80008000 means "no normal" (zero quaternion, a non-finite half among position, quaternion and log-scales).
 * It then composites them over the frame the last encode rasterized with the weights w_i = alpha_i (1 - A) of the colour image: an rgba32f image
 * { N.x, N.y, N.z, A }, N = sum w_i n_i un-normalised (|N| <= A), A bit-identical to WDGS_DEPTH_WEIGHT_SUM.  The words and the image are allocated at
 * the first call, after a change of the point count (words) and of the size (image): such a call cannot be recorded (WDGS_E_STATE); others can.
 * WDGS_E_STATE before encode, and when the forward pass is in point-cloud render mode (no weights).  The two pointers are taken on trust: another
 * cloud, or a camera block rewritten since the forward encode, is NOT detected and gives the normals of a frame that was not composited.  No
 * reference counterpart. */
int wdgs_tiled_rasterizer_encode_normal(wdgs_tiled_rasterizer* op, const void* gaussians_dev, const void* camera_dev);
/* rgba32f[W*H] of the last encode_normal; WDGS_E_STATE before it, and after an encode of another size until the next encode_normal.  No reference counterpart. */
int wdgs_tiled_rasterizer_get_normal(wdgs_tiled_rasterizer* op, void** rgba32f_dev);
/* u32[num_points]: the packed per-Gaussian normals of the last encode_normal; WDGS_E_STATE before it, and after the forward pass changed its point
 * count until the next encode_normal.  No reference counterpart. */
int wdgs_tiled_rasterizer_get_gaussian_normals(wdgs_tiled_rasterizer* op, void** u32_dev);
/* The normals of any f32 depth image, by central differences of its back-projection V(i,j) = (ndc_x z / p00, ndc_y z / p11, z), ndc_x = 2(i+.5)/W - 1,
 * ndc_y = 1 - 2(j+.5)/H (p00 = proj[0][0], p11 = proj[1][1] of the camera block): n = normalize(cross(V(i+1,j) - V(i-1,j), V(i,j+1) - V(i,j-1))),
 * negated where n . V(i,j) > 0.  Writes rgba32f { n, 1 }, and { 0, 0, 0, 0 } where one of the five pixels is outside the image or has a depth that is
 * not > 0 or not finite, or the cross product is zero or not finite.  p00 and p11 finite and non-zero; the output 16-byte aligned.  No reference counterpart. */
int wdgs_depth_to_normals(wdgs_device* dev, const void* depth_f32_dev, uint32_t width, uint32_t height, float p00, float p11, void* normals_rgba32f_dev);
/* How well a composited normal image (get_normal) and a depth-normal image (wdgs_depth_to_normals) agree.  A pixel counts when A >= 0.5, |N| > 0 and
 * the depth normal is valid (w != 0); with c = (N / |N|) . n_d it adds e = rint(A max(1 - c, 0) 2^24) and a = rint(A 2^24).  Writes three uint64
 * { sum e, sum a, pixels } (cleared first; integer atomics, so any order gives the same bits); sum e / sum a is the weight-averaged 1 - cos.
 * Images 16-byte aligned, the sums 8-byte aligned.  No reference counterpart. */
int wdgs_normal_agreement(wdgs_device* dev, const void* normal_rgba32f_dev, const void* depth_normals_rgba32f_dev, uint32_t width, uint32_t height,
                          void* out_u64x3_dev);
/* A normal image as rgba8 for presentation: rgb = round(255 (0.5 + 0.5 (n_x, -n_y, -n_z))), n = N / |N| (a surface that faces the camera is blue),
 * black where |N| is not > 0, alpha 255.  No reference counterpart. */
int wdgs_normal_to_rgba8(wdgs_device* dev, const void* normal_rgba32f_dev, uint32_t width, uint32_t height, void* rgba8_dev);

/* ---------------------------------------------------------------- TiledBackwardPass
 * Replaces `new TiledBackwardPass(device, pointCloud, config)` (renderers/tiled-backward-pass.ts:136-140, config 27-34,
 * TrainingConfig 19-25), .encode (592-740), .computeLossOnly (383), .computeMetricMap (425), .computeMetricCounts (514),
 * .normalizeMetricCounts (565), getters (409-421, 832), .setViewport (742), .setTrainingConfig (812), .destroy (836). */
typedef struct wdgs_training_config {
    float lambda_l1, lambda_l2, lambda_dssim, c1, c2; /* defaults 0.8, 0.0, 0.2, 1e-4, 9e-4 (trainer.ts:100-104) */
} wdgs_training_config;
typedef struct wdgs_tiled_backward_config {
    uint32_t num_points;
    uint32_t sh_deg;
    uint32_t viewport_width, viewport_height;
    wdgs_training_config training;
    float gaussian_scale, point_size_px, max_splat_radius_px;
} wdgs_tiled_backward_config;
typedef struct wdgs_tiled_backward_resources { /* TiledBackwardResources (tiled-backward-pass.ts:40-50) */
    const void* splat_buffer;
    const void* tile_offsets_buffer; /* the RASTERIZER's per-tile table (trainer.ts:621) */
    const void* tile_indices_buffer; /* sorted indices */
    const void* camera_buffer;
    const void* alpha_texture;       /* f32[W*H] final T */
    const void* n_contrib_texture;   /* u32[W*H] */
} wdgs_tiled_backward_resources;

int wdgs_tiled_backward_create(wdgs_device* dev, const wdgs_tiled_backward_config* cfg, wdgs_tiled_backward** out);
/* The point cloud changed size: see wdgs_tiled_forward_resize. */
int wdgs_tiled_backward_resize(wdgs_tiled_backward* op, uint32_t num_points);
int wdgs_tiled_backward_destroy(wdgs_tiled_backward* op);
/* encode: K15 loss gradient, clear accumulators, K16 backward raster, K17 geometry backward -> GaussianGradient[N]. */
int wdgs_tiled_backward_encode(wdgs_tiled_backward* op, const void* predicted_rgba8_dev, const void* target_rgba8_dev,
                               const wdgs_tiled_backward_resources* res, const void* gaussians_dev);
/* The two halves of encode, for a batched step (views_per_rank > 1; no counterpart in the reference, whose step has one view):
 * encode_raster = K15 + clear + K16, encode_geometry = K17.  With `into`, K17 also adds the view's gradient -- the fp16-rounded values
 * it has just packed -- to the step's fp32 block (f32[N][14] + visibility counts, `first` stores instead of adding) and folds the
 * forward pass's overflow word into the step's guard word: what wdgs_store_gradients / wdgs_accumulate_gradients +
 * wdgs_guard_accumulate do in two more launches.  The sums into the block must follow the previous view's (wdgs_device_lane_order). */
typedef struct wdgs_view_accumulate {
    void* sums;                /* f32[N][14] */
    void* visible;             /* u32[N] */
    const void* tile_counts;   /* forward pass: u32[N] */
    void* guard;               /* u32: the step's guard word */
    const void* overflow_word; /* u32: the forward pass's overflow word (stats_buffer + 8) */
    int first;                 /* first view of the step: store, do not add */
} wdgs_view_accumulate;
int wdgs_tiled_backward_encode_raster(wdgs_tiled_backward* op, const void* predicted_rgba8_dev, const void* target_rgba8_dev,
                                      const wdgs_tiled_backward_resources* res);
int wdgs_tiled_backward_encode_geometry(wdgs_tiled_backward* op, const void* camera_dev, const void* gaussians_dev, const wdgs_view_accumulate* into);
int wdgs_tiled_backward_compute_loss_only(wdgs_tiled_backward* op, const void* predicted_rgba8_dev, const void* target_rgba8_dev);
int wdgs_tiled_backward_compute_metric_map(wdgs_tiled_backward* op, const void* predicted_rgba8_dev, const void* target_rgba8_dev, float threshold);
int wdgs_tiled_backward_compute_metric_counts(wdgs_tiled_backward* op, const wdgs_tiled_backward_resources* res, uint32_t num_instances, int clear);
int wdgs_tiled_backward_normalize_metric_counts(wdgs_tiled_backward* op, uint32_t divisor);
int wdgs_tiled_backward_set_viewport(wdgs_tiled_backward* op, uint32_t width, uint32_t height);
int wdgs_tiled_backward_set_training_config(wdgs_tiled_backward* op, const wdgs_training_config* cfg);
/* The loss an encode differentiates (no reference counterpart).  WDGS_DSSIM_REFERENCE (the default): the reference's per-pixel gradient
 * l1 sgn(d) + l2 d + ldssim (1 - SSIM_5x5) d / 2, a 5x5 box window with clamp-to-edge.  WDGS_DSSIM_GAUSSIAN: the exact gradient of
 * sum over pixels and channels of l1 |d| + l2 d^2 / 2 + ldssim (1 - SSIM), SSIM as wdgs_image_ssim_rgb8 defines it (11x11 Gaussian window,
 * zero padding) with the training config's c1 and c2.  Like set_training_config, the mode is read when an encode or
 * compute_loss_only is issued: a recording keeps the loss it was recorded with.  set returns WDGS_E_INVALID for an unknown mode. */
#define WDGS_DSSIM_REFERENCE 0
#define WDGS_DSSIM_GAUSSIAN 1
int wdgs_tiled_backward_set_dssim_mode(wdgs_tiled_backward* op, uint32_t mode);
int wdgs_tiled_backward_get_dssim_mode(const wdgs_tiled_backward* op, uint32_t* out);
void* wdgs_tiled_backward_gradients(wdgs_tiled_backward* op);     /* getGradientsBuffer: GaussianGradient[N] */
void* wdgs_tiled_backward_metric_counts(wdgs_tiled_backward* op); /* getMetricCountsBuffer: u32[N] */
/* computeMetricCounts of this pass adds into `counts_dev` (u32[num_points], e.g. another pass's getMetricCountsBuffer) instead of its own
 * array; NULL restores its own.  No reference counterpart: runDensifyPruneMultiView (trainer.ts:373-497) walks its metric views one after
 * the other through ONE pass; with a shared target several passes can take the views of one densify event on different lanes -- the
 * counts are integer atomics, so every order gives the same bits.  The target must outlive the calls and hold at least num_points words. */
int wdgs_tiled_backward_set_metric_counts_target(wdgs_tiled_backward* op, void* counts_dev);
void* wdgs_tiled_backward_loss_image(wdgs_tiled_backward* op);    /* getLossTextureView: rgba32float W*H */
void* wdgs_tiled_backward_metric_map(wdgs_tiled_backward* op);    /* getMetricMapTextureView: u32[W*H] */
/* Whether the fused step (wdgs_optimizer_step_with_geometry) also writes K17's packed GaussianGradient[N] to the pass's gradient buffer
 * (default 1, as tiled-backward-pass.ts:629-640 does).  A host that never reads getGradientsBuffer() -- trainer.ts hands it to
 * optimizer.step() only, which the fused step replaces -- saves the 32 bytes per Gaussian.  The separate K17 always writes it. */
int wdgs_tiled_backward_set_gradient_output(wdgs_tiled_backward* op, int enabled);
void* wdgs_tiled_backward_accumulators(wdgs_tiled_backward* op);  /* INTERNAL i32[N*12] (for parity tests) */
void* wdgs_tiled_backward_metric_minmax(wdgs_tiled_backward* op); /* u32[2] global (min,max) of the last metric map */
/* Bilinear down-sample of an rgba8 image (the blit render pass of trainer.ts:303-328, shaders/blit.wgsl fs_main). */
int wdgs_downsample_rgba8(wdgs_device* dev, const void* src_dev, uint32_t src_w, uint32_t src_h, void* dst_dev, uint32_t dst_w, uint32_t dst_h);

/* Exact integer sum of squared differences over the R,G,B bytes of two rgba8 images -> *out_u64_dev (u64, device).
 * The reference has no scalar loss (it only visualises the gradient image, trainer.ts:695-768); PSNR = 10 log10(255^2 * 3P / SSE). */
int wdgs_image_sse_rgb8(wdgs_device* dev, const void* a_rgba8_dev, const void* b_rgba8_dev, uint32_t num_pixels, void* out_u64_dev);

/* SSIM of two rgba8 images (W x H, row-major, alpha ignored) -> *out_f64_dev (f64, device): the mean over 3 W H values of the per-pixel, per-channel
 * map of Wang et al. as the 3DGS code base computes it -- values u8/255, 11x11 Gaussian window (sigma 1.5), zero padding, C1 = 0.01^2,
 * C2 = 0.03^2.  map_f32_dev (nullable) receives the map, W*H*3 floats, map[(y*W + x)*3 + c].  Bit-reproducible on one device; identical
 * images give exactly 1.  Stream-ordered, no host wait; may be recorded once a first call on the device (which allocates its fixed
 * scratch) has run outside a recording.  No reference counterpart (held-out evaluation). */
int wdgs_image_ssim_rgb8(wdgs_device* dev, const void* a_rgba8_dev, const void* b_rgba8_dev, uint32_t width, uint32_t height, void* out_f64_dev,
                         void* map_f32_dev);

/* Test hook, not part of the reference's surface: evaluates one pinned arithmetic primitive of the kernels elementwise over
 * `count` 32-bit patterns (0 exp, 1 log, 2 f32->f16 bits, 3 f16 bits->f32, 4 saturating f32->i32, 5 saturating f32->u32,
 * 6 sqrt, 7 1/x), so that a parity suite can compare them with its oracle directly. */
int wdgs_debug_eval_math(wdgs_device* dev, uint32_t which, uint32_t count, const void* in_u32_dev, void* out_u32_dev);

/* Test hook, not part of the reference's surface: runs one route of the forward pass's tile sort on the (key, value) pairs that lie in
 * ping-pong 0 of `s` (key = (tile + 1) << 16 | depth16; the count is stats_dev[0], as always) for a grid of num_tiles_x x num_tiles_y
 * tiles, and writes the per-tile range table into ranges_u32_dev (u32[T + 1], T = num_tiles_x * num_tiles_y: the first index of each
 * tile, 0xFFFFFFFF for an empty one, ranges[T] = count).  route 0: the tile passes on the tile bits + the per-tile depth sort (any grid
 * of 1..65534 tiles); route 1: one pass on the tile row + the per-tile depth sort, for pairs already in tile-column order (2..256
 * columns, <= 256 rows); route 2: the range search alone, on keys the caller has sorted.  The sorted pairs are in
 * ping_pong[final_out_index].  Long tile lists are not built.  WDGS_E_INVALID for a grid the forward pass never asks for. */
int wdgs_debug_sort_tiles(wdgs_sorter* s, uint32_t route, uint32_t num_tiles_x, uint32_t num_tiles_y, void* ranges_u32_dev);

/* Test hook, not part of the reference's surface: composites one frame with the forward pass's rasterize kernel (K14) on tables the caller
 * built -- no projection, no sort.  The settings block and the tile grid are made from viewport, render mode, point size and radius cap by the
 * code a forward pass uses (0 = the default: 128 px cap, 3 px points; a negative cap lifts it).  splats: 6 words per row, num_splats rows
 * count (an entry whose value is >= num_splats is skipped, as the reference skips it); sorted_keys / sorted_vals: the entries, key =
 * (tile + 1) << 16 | depth16, in tile order; count: one device u32, the number of entries; ranges: u32[T + 1], the first entry of each of the
 * T = ceil(w/16) ceil(h/16) tiles, 0xFFFFFFFF for an empty one, ranges[T] = count; max_batches: the compat cap on a tile's list in batches of
 * 256 entries, 0 = none.  nf_stamp == NULL sends every tile through the kernel's EXACT body (the reference's own forms of min, clamp and
 * exp); with nf_stamp (u32[T]) a tile takes it where nf_stamp[tile] == *nf_frame and the fast body elsewhere, so stamps that match nowhere
 * send every tile through the fast body.  Writes the three caller-owned images, W*H elements each: rgba8, final T (f32), n_contrib (u32).
 * No long-list work is passed: long tile lists need the forward pass's own structures and are tested through it (tests/test_gpu_nan.py).
 * WDGS_E_INVALID for a null pointer, an empty viewport, or more tiles than the 16-bit tile field of the key holds. */
typedef struct wdgs_debug_raster_frame {
    uint32_t viewport_width, viewport_height;
    float max_splat_radius_px, point_size_px;
    uint32_t render_mode; /* 1 = gaussian, 0 = point cloud */
    uint32_t num_splats;
    uint32_t max_batches;
    const void* splats;
    const void* sorted_keys;
    const void* sorted_vals;
    const void* count;
    const void* ranges;
    const void* nf_stamp; /* nullable */
    const void* nf_frame; /* nullable when nf_stamp is */
} wdgs_debug_raster_frame;
int wdgs_debug_rasterize(wdgs_device* dev, const wdgs_debug_raster_frame* frame, void* rgba8_dev, void* final_t_dev, void* n_contrib_dev);

/* ---------------------------------------------------------------- Optimizer
 * Replaces allocateOptimizerStateBuffers (renderers/optimizer.ts:27-38), `new Optimizer(device, pointCloud, params?,
 * initialState?)` (71-88), .step (295-350), hyperparameter accessors (256-278), .destroy (352). */
typedef struct wdgs_adam_hyperparameters { /* AdamHyperparameters (renderers/adam-config.ts:1-21) */
    float lr_pos, lr_color, lr_opacity, lr_scale, lr_rot, beta1, beta2, epsilon;
} wdgs_adam_hyperparameters;
typedef struct wdgs_optimizer_state { /* OptimizerStateBuffers (optimizer.ts:13-20); device pointers */
    void* opt_pos;     /* OptVec4[N]   48 B */
    void* opt_rot;     /* OptVec4[N]   48 B */
    void* opt_scale;   /* OptVec4[N]   48 B */
    void* opt_opacity; /* OptFloat[N]  12 B */
    void* param_sh;    /* f32[N*48] */
    void* state_sh;    /* (m,v)[N*48] */
} wdgs_optimizer_state;
/* Byte sizes of the six state arrays for n points, in the struct's field order. */
int wdgs_optimizer_state_sizes(uint32_t num_points, size_t sizes_out[6]);
/* initial_state == NULL: the optimizer allocates zeroed state and initialises the fp32 masters from the fp16 point
 * cloud (K20, optimizer.ts:166-253).  Otherwise the given buffers are ADOPTED as-is (optimizer.ts:81-88) and `owns_state`
 * says whether destroy frees them. */
int wdgs_optimizer_create(wdgs_device* dev, uint32_t num_points, const wdgs_adam_hyperparameters* params,
                          const void* gaussians_dev, const void* sh_dev,
                          const wdgs_optimizer_state* initial_state, int owns_state, uint32_t initial_iteration, wdgs_optimizer** out);
int wdgs_optimizer_destroy(wdgs_optimizer* op);
/* K20 (optimizer.ts:145-253 initBuffers): fp16 point cloud -> fp32 master parameters of this optimizer's state; m, v untouched. */
int wdgs_optimizer_init_from_point_cloud(wdgs_optimizer* op, const void* gaussians_dev, const void* sh_dev);
/* step(encoder, pointCloud, gradientsBuffer, tileCountsBuffer): iteration++, K18 Adam, K19 re-pack into gaussians/sh. */
int wdgs_optimizer_step(wdgs_optimizer* op, void* gaussians_dev, void* sh_dev, const void* gradients_dev, const void* tile_counts_dev);
/* The same step fused with K17: after wdgs_tiled_backward_encode_raster(bwd, ...) for the view, one pass over the Gaussians computes the
 * geometry backward (the packed gradient is still written to bwd's gradient buffer), then Adam and the re-pack of the same Gaussian from
 * the fp16-rounded values in registers -- optimizer.step() of trainer.ts:635 without a second pass over N and a read-back of the gradient. */
int wdgs_optimizer_step_with_geometry(wdgs_optimizer* op, wdgs_tiled_backward* bwd, const void* camera_dev, void* gaussians_dev, void* sh_dev,
                                      const void* tile_counts_dev);
/* Data-parallel variant: gradients are fp32 sums over views, 14 f32 per Gaussian in GaussianGradient
 * component order {pos3, opacity, rot4, logsigma3, rgb3}, plus u32 visibility counts (Adam runs where count > 0). */
int wdgs_optimizer_step_f32(wdgs_optimizer* op, void* gaussians_dev, void* sh_dev, const void* grad_f32_dev, const void* visible_counts_dev);
/* acc_f32[N*14] += unpack(GaussianGradient[N]) where tile_counts > 0; visible[N] += (tile_counts > 0). */
int wdgs_accumulate_gradients(wdgs_device* dev, uint32_t num_points, const void* gradients_dev, const void* tile_counts_dev,
                              void* acc_f32_dev, void* visible_counts_dev);
/* Overwrite form for the first view of a batch: acc_f32[N*14] = unpack(GaussianGradient[N]) (zeros where tile_counts == 0),
 * visible[N] = (tile_counts > 0).  Spares the batch a clearing pass over the 60 B/Gaussian block. */
int wdgs_store_gradients(wdgs_device* dev, uint32_t num_points, const void* gradients_dev, const void* tile_counts_dev,
                         void* acc_f32_dev, void* visible_counts_dev);
/* Adam + re-pack on Gaussians [first, first + count) only: the slice a data-parallel rank owns after
 * wdgs_comm_exchange_gradients.  rows_out_dev (nullable, u32[num_points rounded up][8]) also receives each re-packed row in the
 * 32-byte form {6 Gaussian words, SH word 0, low half of SH word 1} that wdgs_comm_allgather_rows publishes. */
int wdgs_optimizer_step_f32_range(wdgs_optimizer* op, void* gaussians_dev, void* sh_dev, const void* grad_f32_dev, const void* visible_counts_dev,
                                  uint32_t first, uint32_t count, void* rows_out_dev);
/* Writes the rows published by the other ranks into this replica's point cloud: every Gaussian outside [skip_first, skip_first +
 * skip_count).  guard_dev (nullable): non-zero at execution time -> no-op. */
int wdgs_apply_repacked_rows(wdgs_device* dev, uint32_t num_points, const void* rows_dev, uint32_t skip_first, uint32_t skip_count,
                             const void* guard_dev, void* gaussians_dev, void* sh_dev);
/* Guard word: while *flag_u32_dev != 0 at EXECUTION time, step / step_f32 / step_f32_range leave every buffer untouched.  Point it at
 * TiledForwardResources.stats_buffer + 8 (the overflow word): a step whose tile-entry list was truncated -- it will be reported
 * as WDGS_E_CAPACITY by the next wdgs_device_synchronize -- then does not corrupt the optimizer state first.  NULL removes it. */
int wdgs_optimizer_set_guard(wdgs_optimizer* op, const void* flag_u32_dev);
/* Deferred SH writes (no reference counterpart).  update-gaussians.wgsl:59-75 (K19) rewrites the first six bytes of every 96-byte SH row
 * each step; on HBM a 6-byte store is a read-modify-write of a 64-byte memory word.  With deferral on, the step functions write those
 * three fp16 halves to a compact array owned by the optimizer (u32[N][2]: r,g | b,0) and leave the rows alone; a forward pass given that
 * array (wdgs_tiled_forward_set_dc_source) reads the halves from it, so rendering and training see the same values as before.  The rows
 * are brought up to date by wdgs_optimizer_flush_sh, which the host calls at every hand-over: before the cloud's SH buffer is read by the
 * host, exported, rendered by a forward pass that has no dc source (a viewer), or copied by DensifyPrunePass.encodeScatter.
 * `sh_dev` = the point cloud's SH buffer: set_deferred_sh(enabled) takes the current halves from it, (disabled) flushes into it. */
int wdgs_optimizer_set_deferred_sh(wdgs_optimizer* op, void* sh_dev, int enabled);
void* wdgs_optimizer_dc_words(wdgs_optimizer* op);            /* the compact array, or NULL while deferral is off */
int wdgs_optimizer_flush_sh(wdgs_optimizer* op, void* sh_dev); /* no-op unless deferral is on and a step ran since the last flush */
/* wdgs_apply_repacked_rows for a replica whose optimizer defers its SH writes (the gathered halves go to the compact array) */
int wdgs_optimizer_apply_repacked_rows(wdgs_optimizer* op, const void* rows_dev, uint32_t skip_first, uint32_t skip_count, const void* guard_u32_dev,
                                       void* gaussians_dev, void* sh_dev);
/* project_count (K1) takes the SH-DC halves from `dc_words_dev` (wdgs_optimizer_dc_words) instead of the rows; NULL restores the rows */
int wdgs_tiled_forward_set_dc_source(wdgs_tiled_forward* op, const void* dc_words_dev);

/* View-batched step (no reference counterpart: the reference is batch-1, trainer.ts:573).  A step over V views projects every Gaussian
 * for all V cameras in ONE launch -- the 24-byte Gaussian and its 96-byte SH row are read once, not V times -- into the V forward passes'
 * own buffers (`ops[v]`, all created for the same cloud and viewport); each pass then runs the rest of its encode (scan, emit, sort) with
 * wdgs_tiled_forward_encode_projected, on any lane, recorded or not.  Results are those of wdgs_tiled_forward_encode per view, bit for bit. */
int wdgs_tiled_forward_project_views(wdgs_tiled_forward* const* ops, const void* const* cameras_dev, uint32_t count, const void* gaussians_dev, const void* sh_dev);
int wdgs_tiled_forward_encode_projected(wdgs_tiled_forward* op);
/* 1 while the pass holds a projection that wdgs_tiled_forward_encode_projected has not consumed yet and no wdgs_tiled_forward_encode has
 * overwritten (the scan works in place on K1's workgroup sums: the rest of the pass can run once per projection). */
int wdgs_tiled_forward_is_projected(const wdgs_tiled_forward* op);
/* ... and K17 of all V views in one launch: per view the accumulators of `ops[v]` (wdgs_tiled_backward_encode_raster ran for it) are turned
 * into the view's fp16 gradient under `cameras_dev[v]` and summed, in view order, into the step's fp32 block `sums_f32_dev` [N][14] with the
 * visibility counts `visible_dev` [N] and the guard word (OR of the views' overflow words `overflow_words_dev[v]`) -- what V calls of
 * wdgs_tiled_backward_encode_geometry(into = {first: v == 0}) produce, bit for bit, with the Gaussians read once and the fp32 block written
 * once.  `write_gradients` != 0 also stores each view's packed gradient in its pass's gradient buffer.  A step may hand its views over
 * in several GROUPS (so that one group's K17 runs beside the next group's rasterization): `continues` = 0 for the group that holds the
 * step's first view, 1 for every later group, in view order -- the block then goes on from what the earlier groups left. */
int wdgs_tiled_backward_encode_geometry_views(wdgs_tiled_backward* const* ops, const void* const* cameras_dev, const void* const* tile_counts_dev,
                                              const void* const* overflow_words_dev, uint32_t count, const void* gaussians_dev, void* sums_f32_dev,
                                              void* visible_dev, void* guard_u32_dev, int write_gradients, int continues);
/* flag = (overwrite ? 0 : flag) | (*src != 0): folds the overflow words of the views of a batched step into one guard word. */
int wdgs_guard_accumulate(wdgs_device* dev, void* flag_u32_dev, const void* src_u32_dev, int overwrite);
/* The caller rewrote the state arrays (gathered slices from other ranks): refresh the optimizer's internal compact copies. */
int wdgs_optimizer_state_changed(wdgs_optimizer* op);
uint32_t wdgs_optimizer_get_iteration(const wdgs_optimizer* op);
/* Host-side counter only (optimizer.ts:301): call when a recorded command buffer containing step() is re-submitted. */
int wdgs_optimizer_advance_iteration(wdgs_optimizer* op, uint32_t count);
int wdgs_optimizer_get_hyperparameters(const wdgs_optimizer* op, wdgs_adam_hyperparameters* out);
int wdgs_optimizer_set_hyperparameters(wdgs_optimizer* op, const wdgs_adam_hyperparameters* params);
/* getStateBuffers.  The optimizer trains a compact copy of the SH-DC parameter and moments (36 B per Gaussian instead of
 * three cache lines at 192/384-byte strides); param_sh / state_sh rows 0..2 are brought up to date HERE, in
 * wdgs_optimizer_release_state and in wdgs_optimizer_destroy (adopted state).  Always fetch the state through one of these
 * before reading those two arrays or handing them to wdgs_densify_prune_encode_scatter. */
int wdgs_optimizer_get_state(wdgs_optimizer* op, wdgs_optimizer_state* out);
/* Detaches the state so destroy does not free it (hand-over across a densify swap, trainer.ts:492-495). */
int wdgs_optimizer_release_state(wdgs_optimizer* op, wdgs_optimizer_state* out);

/* ---------------------------------------------------------------- DensifyPrunePass
 * Replaces `new DensifyPrunePass(device, config)` (renderers/densify-prune.ts:108, config 17-30), .setConfig/.ensureSize
 * (279-312), .encodePrepare (458-468: decide K26, scan, cap K27, scan, total K28), .encodeScatter (470-678: K29 + K30). */
typedef struct wdgs_densify_config {
    uint32_t num_views;              /* numViews */
    uint32_t clone_threshold;        /* cloneThreshold (metric count) */
    float split_threshold;           /* splitThreshold (max scale) */
    float prune_threshold;           /* pruneThreshold (opacity) */
    uint32_t max_new_points_per_step;/* 0 = unlimited */
    uint64_t max_buffer_bytes;       /* 128 MiB in the reference; 0 = unlimited */
} wdgs_densify_config;
typedef struct wdgs_densify_prepared { /* DensifyPrunePrepared (densify-prune.ts:42-48) */
    void* action_buffer;     /* u32[N] 0 keep, 1 clone, 2 split, 3 prune */
    void* out_count_buffer;  /* u32[N] */
    void* out_offset_buffer; /* u32[N] exclusive scan */
    void* out_total_buffer;  /* u32[1] */
    uint32_t max_out_points;
} wdgs_densify_prepared;

int wdgs_densify_prune_create(wdgs_device* dev, const wdgs_densify_config* cfg, wdgs_densify_prune** out);
int wdgs_densify_prune_destroy(wdgs_densify_prune* op);
int wdgs_densify_prune_set_config(wdgs_densify_prune* op, const wdgs_densify_config* cfg);
int wdgs_densify_prune_ensure_size(wdgs_densify_prune* op, uint32_t num_points);
int wdgs_densify_prune_encode_prepare(wdgs_densify_prune* op, uint32_t num_points, const void* gaussians_dev,
                                      const void* metric_counts_dev, wdgs_densify_prepared* out);
/* The stages encodePrepare is made of, individually recordable as in the reference: .encodeDecision (densify-prune.ts:412-456,
 * K26), .encodePrefixSum (327-337: exclusive scan of out_count into out_offset), .encodeCapToMax (363-388, K27),
 * .encodeTotalOut (339-361, K28) and computeMaxOutPoints (390-410).  The work buffers are the ones encode_prepare reports. */
int wdgs_densify_prune_encode_decision(wdgs_densify_prune* op, uint32_t num_points, const void* gaussians_dev, const void* metric_counts_dev);
int wdgs_densify_prune_encode_prefix_sum(wdgs_densify_prune* op, uint32_t num_points);
int wdgs_densify_prune_encode_cap_to_max(wdgs_densify_prune* op, uint32_t num_points, uint32_t max_out_points);
int wdgs_densify_prune_encode_total_out(wdgs_densify_prune* op, uint32_t num_points);
int wdgs_densify_prune_compute_max_out_points(wdgs_densify_prune* op, uint32_t num_points, uint32_t* max_out_points);
/* getOutTotalBuffer & co. (densify-prune.ts:314-324): the pass's work buffers; WDGS_E_STATE before they exist. */
int wdgs_densify_prune_get_buffers(wdgs_densify_prune* op, wdgs_densify_prepared* out);
/* Reads the 4-byte total back (the one device->host crossing of the densify path, trainer.ts:440-458). */
int wdgs_densify_prune_read_total(wdgs_densify_prune* op, uint32_t* total_out);
/* Contribution-based pruning.  No reference counterpart.  A decision stage in place of encode_decision that reads the
 * records wdgs_tiled_rasterizer_encode_contribution accumulated: a Gaussian is KEPT iff it meets every non-zero field of the rule -- max weight >=
 * min_max_weight, sum_q * 2^-24 >= min_weight_sum (compared in float64), pixels >= min_pixels, sum_q >= min_sum_q.  Writes action_buffer (0 keep,
 * 3 prune) and out_count_buffer (1 or 0); encode_prefix_sum, encode_total_out, read_total and encode_scatter then compact the cloud, the SH rows
 * and the optimizer arrays.  A Gaussian this stage keeps is copied by the next encode_scatter bit for bit (the densify decision's survivors have
 * their opacity clamped and its moments reset, densify-prune-scatter; here nothing but the pruned rows may change).  An all-zero rule is
 * WDGS_E_INVALID. */
typedef struct wdgs_contribution_rule {
    float min_max_weight;
    float min_weight_sum;
    uint32_t min_pixels;
    uint64_t min_sum_q;
} wdgs_contribution_rule;
int wdgs_densify_prune_encode_contribution_decision(wdgs_densify_prune* op, uint32_t num_points, const void* stats_dev, const wdgs_contribution_rule* rule);
/* encodeScatter: out_num_points must equal the size of the output buffers (the reference throws otherwise,
 * densify-prune.ts:478-480).  in_state/out_state may both be NULL (point cloud only). */
int wdgs_densify_prune_encode_scatter(wdgs_densify_prune* op, uint32_t in_points, const void* in_gaussians_dev, const void* in_sh_dev,
                                      const wdgs_optimizer_state* in_state, uint32_t out_num_points, int reset_new_optimizer_state,
                                      void* out_gaussians_dev, void* out_sh_dev, const wdgs_optimizer_state* out_state);

/* ---------------------------------------------------------------- data-parallel communicator (RCCL over xGMI)
 * No counterpart in the reference, which trains one view per step on one GPU (trainer.ts:573).  View-sharded data parallelism
 * (SURVEY 8(e)): every rank holds a full replica, runs K1-K17 on its own views, sums GaussianGradients into acc_f32[N*14] +
 * visible[N] (wdgs_accumulate_gradients), all-reduces both, and applies wdgs_optimizer_step_f32 -- identical on every rank,
 * so replicas stay bit-identical; world_size = 1 reduces to the reference step.  One process (or host thread) per GPU: rank 0
 * calls wdgs_comm_get_unique_id and ships the 128 bytes to the others over any host channel; all ranks then call
 * wdgs_comm_create.  Reductions are queued on the device's stream (no host sync).  RCCL is bound lazily, on first use. */
#define WDGS_COMM_ID_BYTES 128
typedef struct wdgs_comm wdgs_comm;
int wdgs_comm_get_unique_id(uint8_t id_out[WDGS_COMM_ID_BYTES]);
int wdgs_comm_create(wdgs_device* dev, const uint8_t id[WDGS_COMM_ID_BYTES], int world_size, int rank, wdgs_comm** out);
int wdgs_comm_destroy(wdgs_comm* comm);
int wdgs_comm_world_size(const wdgs_comm* comm);
int wdgs_comm_rank(const wdgs_comm* comm);
/* In place: grad_f32[N*14] (f32 sum) and visible_counts[N] (u32 sum) over all ranks, one RCCL group. */
int wdgs_comm_allreduce_gradients(wdgs_comm* comm, void* grad_f32_dev, void* visible_counts_dev, uint32_t num_points);
/* In place u32 sum (densify metric counts, SURVEY 8(e) "Determinism"). */
int wdgs_comm_allreduce_counts(wdgs_comm* comm, void* counts_u32_dev, uint32_t count);
/* The bandwidth-optimal form of the same exchange: reduce-scatter -> Adam on the owned slice -> all-gather of the
 * re-packed rows.  Gaussians are dealt to ranks in contiguous slices of slice_points = ceil(N / world_size) rounded up to 64; rank r
 * owns [r*slice, min((r+1)*slice, N)).  grad_f32_dev and visible_counts_dev hold world_size*slice_points rows (tail zero); after the
 * call rank r's OWN slice holds the sums over all ranks (the other slices are scratch).  flag_u32_dev (nullable, one u32) is summed
 * over all ranks in the same RCCL group: a per-rank "tile entries overflowed" word becomes a global one, so every rank skips the
 * step together (wdgs_optimizer_set_guard).  Then wdgs_optimizer_step_f32_range(first = r*slice, rows_out = rows) and
 * wdgs_comm_allgather_rows(rows) (in place, world_size*slice_points rows of 32 bytes) and wdgs_apply_repacked_rows.  Per step and
 * rank this moves (7/8)(60 + 32) B per Gaussian instead of the all-reduce's 2(7/8)60 B, and divides the Adam pass by world_size.
 * The optimizer state of a slice lives on its owner; gather it with wdgs_comm_broadcast (one call per owner and array, optionally
 * inside wdgs_comm_group_start/end) + wdgs_optimizer_state_changed before a densify rebuild or an export. */
int wdgs_comm_exchange_gradients(wdgs_comm* comm, void* grad_f32_dev, void* visible_counts_dev, void* flag_u32_dev, uint32_t slice_points);
int wdgs_comm_allgather_rows(wdgs_comm* comm, void* rows_dev, uint32_t slice_points);
int wdgs_comm_broadcast(wdgs_comm* comm, void* ptr_dev, size_t bytes, int root);
int wdgs_comm_group_start(void);
int wdgs_comm_group_end(void);

/* ---------------------------------------------------------------- TSDF volume: fusion of depth maps and a triangle mesh
 * The reference renders colour only and has no counterpart to any of the ten entries below.  The volume is an axis-aligned grid of nx x ny x nz voxels in
 * world space, x fastest: voxel (i, j, k) has the linear index (k ny + j) nx + i and its centre at origin + (i + 1/2, j + 1/2, k + 1/2) voxel_size.  It holds
 * tsdf f32 (in units of `truncation`, 1 = free or unseen) and weight f32 per voxel and, with `colour` != 0, rgb as three f32 planes (r, g, b; nx ny nz floats
 * each).  create allocates everything the other entries use, and resets.  WDGS_E_INVALID when a dimension is < 2, nx ny nz > 2^28 (the mesh has at most 12
 * triangles per cell: their u32 count cannot overflow), voxel_size or truncation is not positive and finite, max_weight is not >= 1, or the origin is not finite.
 * No reference counterpart. */
typedef struct wdgs_tsdf_volume wdgs_tsdf_volume;
int wdgs_tsdf_volume_create(wdgs_device* dev, const float* origin3, float voxel_size, uint32_t nx, uint32_t ny, uint32_t nz, float truncation, float max_weight,
                            uint32_t colour, wdgs_tsdf_volume** out);
int wdgs_tsdf_volume_destroy(wdgs_tsdf_volume* vol);
/* tsdf = 1, weight = 0, rgb = 0; stream-ordered, recordable.  No reference counterpart. */
int wdgs_tsdf_volume_reset(wdgs_tsdf_volume* vol);
/* The device arrays: f32[nx ny nz], f32[nx ny nz], f32[3][nx ny nz] (WDGS_E_STATE for a volume without colour).  A host may write through them, so each call
 * counts as a write of the volume for emit_triangles' state rule.  No reference counterpart. */
int wdgs_tsdf_volume_get_tsdf(wdgs_tsdf_volume* vol, void** f32_dev);
int wdgs_tsdf_volume_get_weight(wdgs_tsdf_volume* vol, void** f32_dev);
int wdgs_tsdf_volume_get_rgb(wdgs_tsdf_volume* vol, void** f32x3_dev);
int wdgs_tsdf_volume_get_dims(const wdgs_tsdf_volume* vol, uint32_t* dims3);
/* Fuses ONE view: a pass over the volume, one thread per voxel, no atomics, f32 in the order given here.  For a voxel centre c: v = view (c, 1) from the 68-float
 * camera block (view = floats 0-15, column-major; products summed left to right), z = v.z, skipped unless z > 0; px = (((P00 v.x) / z) / 2 + 1/2) W,
 * py = ((((-P11) v.y) / z) / 2 + 1/2) H (P00 = block[32], P11 = block[37]), the pixel (floor px, floor py), skipped outside the image; d the depth there, skipped
 * unless d > 0 and finite, and -- with a weight-sum image -- unless its value there is >= min_weight_sum; sdf = d - z, skipped if sdf < -truncation;
 * t = min(sdf / truncation, 1); then T = (T Wt + t) / (Wt + 1), each colour plane likewise from the pixel's byte / 255 when a colour image is given, and
 * Wt = min(Wt + 1, max_weight).  A skipped voxel is not written.  The result depends only on the order of the calls.  weight_sum and colour are nullable.
 * WDGS_E_STATE when colour is given to a volume without colour, and when width, height disagree with the block's floats 64-65: an eager call reads those two
 * back (a host wait); a call recorded into a command buffer cannot, and writes nothing when they disagree.  No allocation: recordable.  No reference counterpart. */
int wdgs_tsdf_volume_integrate(wdgs_tsdf_volume* vol, const void* depth_f32_dev, const void* weight_sum_f32_dev, const void* colour_rgba8_dev, uint32_t width,
                               uint32_t height, const void* camera_dev, float min_weight_sum);
/* Marching tetrahedra over the cells (i, j, k), 0 <= i < nx - 1 and likewise, whose eight corner voxels all have weight >= min_weight (> 0, finite): each cell is cut
 * into the six tetrahedra {0, e_a, e_a + e_b, (1,1,1)} of the axis permutations xyz, xzy, yxz, yzx, zxy, zyx; a corner is inside when T < 0 (0 is outside); one or
 * three inside corners give one triangle, two give two, wound counter-clockwise seen from the outside.  count_triangles counts per cell, scans, waits and returns
 * the total; it cannot be recorded (WDGS_E_STATE).  No reference counterpart. */
int wdgs_tsdf_volume_count_triangles(wdgs_tsdf_volume* vol, float min_weight, uint32_t* total);
/* Writes the `total` triangles of the last count_triangles -- cells in linear order, then tetrahedron order, then triangle order -- as
 * positions f32[total][3][3], keys u64[total][3] (nullable) and colours rgba8[total][3] (nullable; alpha 255).  A vertex lies on the lattice edge between the
 * corners A and B, A the one of lower linear index: p = pA + (pB - pA) (T_A / (T_A - T_B)), key = linear_index(A) 8 + (dx + 2 dy + 4 dz - 1) with (dx, dy, dz) the
 * offset from A to B; equal keys have equal position bits.  WDGS_E_CAPACITY when capacity_triangles < total (nothing is written); WDGS_E_STATE when no count
 * precedes it, when the volume was integrated, reset or handed out by a getter since the count (the replay of a recorded integrate is not seen), and when colours
 * are asked of a volume without colour.  No reference counterpart. */
int wdgs_tsdf_volume_emit_triangles(wdgs_tsdf_volume* vol, void* positions_f32_dev, void* keys_u64_dev, void* colours_rgba8_dev, uint32_t capacity_triangles);

/* ---------------------------------------------------------------- Mesh accuracy metrics: surface sampling, nearest points, distance sums
 *
 * Three device pieces, each defined so that a float32 restatement reproduces its output bit for bit (every f32 operation rounded once in the order written,
 * sums as integers).  No reference counterpart. */

/* Area-weighted sampling of a triangle mesh: vertices f32[V][3], faces u32[F][3], `density` samples per unit area (positive, finite), a u32 seed.
 *   mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16                      (u32, wrapping)
 *   h(seed, t, k, j) = mix(mix(mix(mix(seed + 0x9E3779B9) ^ t) + k) ^ (j * 0x85EBCA6B + 1));   unit(h) = ((float)(h >> 9) + 0.5f) * 2^-23
 * Triangle t with corners A, B, C: e1 = B - A, e2 = C - A, n = e1 x e2, area = 0.5f sqrt((n.x n.x + n.y n.y) + n.z n.z), and it gets
 * n_t = u32(floor(area density + unit(h(seed, t, 0xFFFFFFFF, 0)))) samples, at most 2^31 - 1; 0 when it names a vertex >= V or the sum is not finite.
 * Sample k of triangle t is output element offsets[t] + k (offsets: the exclusive scan of n_t): u = unit(h(seed, t, k, 1)), v = unit(h(seed, t, k, 2)),
 * both replaced by 1 - u, 1 - v when u + v > 1, and per axis p = (A + u e1) + v e2. */
typedef struct wdgs_mesh_sampler wdgs_mesh_sampler;
int wdgs_mesh_sampler_create(wdgs_device* dev, wdgs_mesh_sampler** out);
int wdgs_mesh_sampler_destroy(wdgs_mesh_sampler* sampler);
/* Counts and scans; waits for the u64 total and returns it, so it cannot be recorded (WDGS_E_STATE).  WDGS_E_CAPACITY for a total of 2^31 or more: no emit
 * is possible after it.  The mesh is read again by the emit and must stay as it is until then. */
int wdgs_mesh_sampler_count(wdgs_mesh_sampler* sampler, const void* vertices_f32_dev, uint32_t num_vertices, const void* faces_u32_dev, uint32_t num_faces, float density,
                            uint32_t seed, uint64_t* total);
/* Writes points f32[total][3] and face u32[total] (nullable: the triangle of each sample), one thread per sample.  WDGS_E_STATE unless the last count
 * succeeded with these very arguments; WDGS_E_CAPACITY when capacity_samples < total; nothing is written in either case.  Stream-ordered, recordable. */
int wdgs_mesh_sampler_emit(wdgs_mesh_sampler* sampler, const void* vertices_f32_dev, uint32_t num_vertices, const void* faces_u32_dev, uint32_t num_faces, float density,
                           uint32_t seed, void* points_f32_dev, void* face_u32_dev, uint32_t capacity_samples);

/* A uniform grid over points f32[M][3] (M <= 2^31 - 1, else WDGS_E_INVALID; M = 0 is allowed) holding a cell-sorted copy of the finite points as 16-byte records
 * { x, y, z, original index }; non-finite points are left out.  The build reads the points' bounds back with one wait and cannot be recorded (WDGS_E_STATE); the
 * points are not read after it.  cell_size: the cell edge, a speed parameter only -- no result depends on it; the library enlarges it until the grid has at most
 * 2^26 cells; 0 = chosen by the first query, which then completes the build (and cannot be recorded either; the points must be unchanged until then): its
 * cutoff, or w / cbrt(n) if that is smaller (w the widest extent of the n finite points: a cube of that extent then has n cells). */
typedef struct wdgs_point_index wdgs_point_index;
int wdgs_point_index_create(wdgs_device* dev, const void* points_f32_dev, uint64_t num_points, float cell_size, wdgs_point_index** out);
int wdgs_point_index_destroy(wdgs_point_index* index);
/* Room for queries of up to num_queries points.  A query grows the room by itself except while recording, where it fails with WDGS_E_STATE instead. */
int wdgs_point_index_reserve_queries(wdgs_point_index* index, uint32_t num_queries);
/* The cell edge in use (0 before the grid exists), the grid's dimensions and the number of points indexed; each pointer nullable. */
int wdgs_point_index_info(const wdgs_point_index* index, float* cell_size, uint32_t* dims3, uint32_t* indexed_points);
/* For each query p of queries f32[K][3]: over the indexed points q with d2(p, q) = ((dx dx + dy dy) + dz dz) <= r2, dx = p.x - q.x ..., r2 = max_distance
 * max_distance (all f32), the smallest d2 and, among equal d2, the lowest original index, into d2 f32[K] and index u32[K]; +inf and 0xFFFFFFFF when there is none
 * or the query is not finite.  pairs_u64_dev (nullable): the number of (query, point) pairs examined is added to it.  max_distance must be positive and finite
 * (WDGS_E_INVALID).  Stream-ordered, recordable once the grid exists and the room is reserved. */
int wdgs_point_index_nearest(wdgs_point_index* index, const void* queries_f32_dev, uint32_t num_queries, float max_distance, void* d2_f32_dev, void* index_u32_dev,
                             void* pairs_u64_dev);
/* The bounding box of the finite points as the build read it back: lo f32[3] and hi f32[3], each nullable; all zero when no point is finite.  No device work. */
int wdgs_point_index_bounds(const wdgs_point_index* index, float* lo3, float* hi3);
/* The k nearest.  For query i of queries f32[K][3] the candidates are the indexed points j with d2 <= r2 (d2, r2 as for nearest), with
 * WDGS_KNN_EXCLUDE_SELF only those with original index j != i -- the self-query, where the queries are the indexed points.  Ordered by (d2, j), the lower index
 * first among equal d2, the first min(k, count) of them go to slots 0 .. of row i of d2 f32[K][k] and index u32[K][k]; the remaining slots, and every slot of a
 * non-finite query, receive +inf and 0xFFFFFFFF.  1 <= k <= WDGS_KNN_MAX_K, K k <= 2^32 - 1, max_distance positive and finite, no unknown flag bit
 * (WDGS_E_INVALID; nothing is written).  pairs_u64_dev and recording as for nearest; with k = 1 and no flag the outputs and the pair count are nearest's. */
#define WDGS_KNN_EXCLUDE_SELF 1u
#define WDGS_KNN_MAX_K 16u
int wdgs_point_index_k_nearest(wdgs_point_index* index, const void* queries_f32_dev, uint32_t num_queries, uint32_t k, float max_distance, uint32_t flags,
                               void* d2_f32_dev, void* index_u32_dev, void* pairs_u64_dev);
/* positions f32[N][3] = halves 0, 1, 2 (fp16) of each record of gaussians u32[N][6], exactly: the positions the renderer sees.  Stream-ordered, recordable. */
int wdgs_point_cloud_positions(wdgs_device* dev, const void* gaussians_dev, uint32_t num_points, void* positions_f32_dev);
/* 3DGS's scale initialisation from k_nearest's d2 f32[N][k] of a self-query.  Per point: found = the finite slots, s = their f32 sum from slot 0 on,
 * mean = s / (float)found, log sigma = 0.5f log(max(mean, min_d2)) (the library's log, DESIGN.md "dmath"), rounded to fp16 (nearest even) into halves 8, 9, 10
 * of its record; half 11 and halves 0 - 7 keep their bytes.  A point with found = 0 keeps its whole record.  mean_d2 f32[N] (nullable) receives mean, +inf for
 * found = 0.  min_d2 positive and finite, 1 <= k <= WDGS_KNN_MAX_K (WDGS_E_INVALID).  Stream-ordered, recordable. */
int wdgs_point_cloud_neighbour_scales(wdgs_device* dev, void* gaussians_dev, uint32_t num_points, const void* d2_f32_dev, uint32_t k, float min_d2,
                                      void* mean_d2_f32_dev);
/* out u64[3] = { n_found: the finite d2;  n_within: those with d2 <= threshold threshold (f32);  sum_q: the sum over the found of
 * u32((sqrt(d2) / max_distance) * 2^24) }, exact integer sums; the mean distance is sum_q max_distance / 2^24 / n_found.  0 < threshold <= max_distance, both
 * finite (WDGS_E_INVALID).  Stream-ordered, no host wait, recordable. */
int wdgs_point_distance_stats(wdgs_device* dev, const void* d2_f32_dev, uint32_t count, float max_distance, float threshold, void* out_u64x3_dev);

/* ---------------------------------------------------------------- Mesh connected components and small-component removal
 *
 * Input: an indexed mesh, faces u32[F][3] over V vertices, 0 <= F, V < 2^31.  A face is VALID when its three indices are < V.  An invalid face joins nothing,
 * is counted in invalid_faces, gets the component 0xFFFFFFFF, is never kept and never read as an address.  Degenerate faces such as (a, a, a) and (a, a, b) are
 * valid and connect what they name.  Two vertices are CONNECTED when a valid face names both, taken transitively: connectivity through shared vertices (two
 * cones that touch at one vertex are one component), not through shared edges.  A COMPONENT is a connectivity class that holds at least one valid face; its
 * representative is its lowest vertex index, and components are numbered 0 .. C - 1 in ascending order of representative.  A vertex that no valid face names
 * belongs to no component (0xFFFFFFFF).  Outputs: face_component u32[F], vertex_component u32[V], triangles u32[C] and vertices u32[C] (the valid faces and the
 * vertices of each component), C and invalid_faces -- each a function of the input alone, bit for bit, whatever the launch geometry or the order in which
 * threads ran (a lock-free union-find that links the larger root under the smaller; integer atomics only).  No reference counterpart. */
typedef struct wdgs_mesh_components wdgs_mesh_components;
int wdgs_mesh_components_create(wdgs_device* dev, wdgs_mesh_components** out);
int wdgs_mesh_components_destroy(wdgs_mesh_components* components);
/* Labels the mesh into arrays the object owns (it grows them as needed).  Waits once, to read C and invalid_faces, so it cannot be recorded (WDGS_E_STATE).
 * WDGS_E_INVALID for null faces with num_faces != 0 and for num_faces or num_vertices >= 2^31.  The faces are read again by compact and must stay as they are
 * until then. */
int wdgs_mesh_components_label(wdgs_mesh_components* components, const void* faces_u32_dev, uint32_t num_faces, uint32_t num_vertices, uint32_t* num_components,
                               uint32_t* invalid_faces);
/* The device arrays of the last label (each pointer nullable; an array of no elements is handed out as null): valid until the next label or destroy, complete
 * once the stream has run.  WDGS_E_STATE when no label precedes it.  No device work. */
int wdgs_mesh_components_get(wdgs_mesh_components* components, void** face_component_u32_dev, void** vertex_component_u32_dev, void** triangles_u32_dev,
                             void** vertices_u32_dev);
/* Chooses the components to keep: keep_host u8[C], non-zero = kept, C the last label's count (WDGS_E_INVALID otherwise).  A face is kept when its component is;
 * a vertex is kept exactly when its component is.  Flags and scans both, waits and returns the numbers of kept vertices and faces; cannot be recorded
 * (WDGS_E_STATE, also when no label precedes it). */
int wdgs_mesh_components_select(wdgs_mesh_components* components, const uint8_t* keep_host, uint32_t num_components, uint32_t* kept_vertices, uint32_t* kept_faces);
/* Writes the kept part of the mesh for the last select: kept faces in their original order with their indices rewritten to the new numbering, faces_out
 * u32[F'][3]; kept vertices in ascending original index, vertices_out f32[V'][3] gathered from vertices f32[V][3] (both nullable together: no positions);
 * vertex_map u32[V'] and face_map u32[F'] (each nullable), the old index of each new vertex and face.  WDGS_E_CAPACITY, with nothing written, when
 * capacity_vertices < V' or capacity_faces < F'; WDGS_E_STATE when no select precedes it.  Stream-ordered, no host wait, recordable. */
int wdgs_mesh_components_compact(wdgs_mesh_components* components, const void* vertices_f32_dev, void* vertices_out_f32_dev, void* faces_out_u32_dev,
                                 void* vertex_map_u32_dev, void* face_map_u32_dev, uint32_t capacity_vertices, uint32_t capacity_faces);

/* ---------------------------------------------------------------- Welding a triangle soup: a stable u64 key sort, head flags, a scan, a gather
 *
 * Input: S = 3 F slots, 0 <= S < 2^32 (anything else: WDGS_E_INVALID), with keys u64[S], positions f32[S][3] and (optional) colours rgba8[S] on the device -- the
 * layout emit_triangles writes.  Keys are arbitrary u64; 0 and 2^64 - 1 are keys like any other.  Outputs: V, the number of distinct keys; keys_out u64[V], the
 * distinct keys ascending; vertices f32[V][3] and colours rgba8[V], for every distinct key the bits of the LOWEST slot that carries it (also where equal keys carry
 * different positions); faces u32[S], for every slot the rank of its key among the distinct keys.  Each is a function of the input alone, bit for bit, whatever the
 * launch geometry or the order in which threads ran: a stable least-significant-digit radix sort of (key, slot) pairs by 8-bit digits, each pass a histogram, a scan
 * and a scatter in launches of their own, and no workgroup ever waits for another.  A pass whose digit is the same in every key is skipped.  No reference counterpart. */
typedef struct wdgs_mesh_welder wdgs_mesh_welder;
int wdgs_mesh_welder_create(wdgs_device* dev, wdgs_mesh_welder** out);
int wdgs_mesh_welder_destroy(wdgs_mesh_welder* welder);
/* Sorts the pairs into arrays the object owns (it grows them as needed: 32 bytes per slot), flags the heads and scans them.  Waits once, to read V, so it cannot be
 * recorded (WDGS_E_STATE).  WDGS_E_INVALID for num_slots >= 2^32 or no multiple of 3 and for null keys with num_slots != 0.  The keys are read again by emit when
 * no pass ran and must stay as they are until then. */
int wdgs_mesh_welder_count(wdgs_mesh_welder* welder, const void* keys_u64_dev, uint64_t num_slots, uint32_t* num_vertices);
/* Writes the outputs of the last count: faces_out u32[S]; keys_out u64[V] (nullable); vertices_out f32[V][3] gathered from positions (nullable together);
 * colours_out rgba8[V] gathered from colours (nullable together).  WDGS_E_STATE unless the last count succeeded with these very keys and num_slots;
 * WDGS_E_CAPACITY when capacity_vertices < V; nothing is written in either case.  Stream-ordered, no host wait, recordable. */
int wdgs_mesh_welder_emit(wdgs_mesh_welder* welder, const void* keys_u64_dev, uint64_t num_slots, const void* positions_f32_dev, const void* colours_rgba8_dev,
                          void* keys_out_u64_dev, void* vertices_out_f32_dev, void* colours_out_rgba8_dev, void* faces_out_u32_dev, uint32_t capacity_vertices);
/* The last count: the radix passes that ran and those skipped (eight in all), V and S; each pointer nullable.  WDGS_E_STATE when no count precedes it.  The
 * kernels' event times are the device's (wdgs_device_get_kernel_times): weld_key_bits, weld_plan, weld_histogram, weld_scatter, weld_heads, weld_emit and the
 * scan's three.  No device work. */
int wdgs_mesh_welder_stats(const wdgs_mesh_welder* welder, uint32_t* passes_run, uint32_t* passes_skipped, uint32_t* num_vertices, uint32_t* num_slots);

/* ---------------------------------------------------------------- Mesh simplification by vertex clustering
 *
 * Input: an indexed mesh on the device, vertices f32[V][3], faces u32[F][3], optional colours rgba8[V], 0 <= V, F < 2^31 (WDGS_E_INVALID otherwise).  Parameters:
 * origin f32[3], finite, and cell_size, an f32 that is finite and > 0 (anything else: WDGS_E_INVALID); inv = 1.0f / cell_size is formed once on the host in f32
 * and no kernel divides floats.
 * CELLS.  Per axis t = (p - origin) * inv and c = floorf(t), each operation rounded once.  A vertex is INSIDE when all three t are finite and all three c satisfy
 * 0 <= c < 2^21; its key is cz 2^42 | cy 2^21 | cx.  An OUTSIDE vertex has the key 2^64 - 1 and belongs to no cluster.  The CLUSTERS are the distinct inside
 * keys, numbered 0 .. C - 1 in ascending key order.
 * REPRESENTATIVE, integers only.  Per axis and vertex q = u32((t - c) * 65536.0f) (the subtraction is exact, the conversion truncates); Q the sum of q over the
 * cluster's n vertices as a u64; Qm = (2 Q + n) / (2 n) in unsigned integer division; the position is origin + (f32(c) + (f32(Qm) + 0.5f) * 2^-16) * cell_size,
 * each operation rounded once in that order.  Each of the four colour bytes alike: (2 sum + n) / (2 n).  No float is ever summed, so nothing depends on the order
 * in which threads ran.  Positions are thereby re-quantised to cell_size 2^-16: the result is NOT the identity however small the cell.
 * FACES.  A face is dropped, and counted in exactly one class, in this order of precedence: INVALID, an index >= V (never read as an address); OUTSIDE, it names
 * an outside vertex; COLLAPSED, two of its corners fall in one cluster; DUPLICATE, a face of lower index has the same three clusters in the same cyclic order
 * (rotate each face so that its smallest cluster comes first and compare the triples: (a, b, c) and (a, c, b) are different faces and both stay).  Kept faces stay
 * in input order with their corners in input order, rewritten to the new vertex numbering.  A cluster is emitted as a vertex exactly when a kept face names it;
 * emitted vertices are in ascending key order.
 * OUTPUTS.  V', F'; vertices_out f32[V'][3]; colours_out rgba8[V'] (with colours); keys_out u64[V'], the cell keys; faces_out u32[F'][3]; face_map u32[F'], the
 * old face of each new one; vertex_cluster u32[V], the new index of each old vertex or 0xFFFFFFFF when it has none; the counts C, invalid, outside, collapsed,
 * duplicate.  Each is a function of the input alone, bit for bit.  No reference counterpart. */
typedef struct wdgs_mesh_simplifier wdgs_mesh_simplifier;
int wdgs_mesh_simplifier_create(wdgs_device* dev, wdgs_mesh_simplifier** out);
int wdgs_mesh_simplifier_destroy(wdgs_mesh_simplifier* simplifier);
/* Everything up to the final scans, into arrays the object owns (it grows them as needed: about 130 bytes per vertex and 70 per face): cell keys, three stable
 * sorts (the weld's: the vertices' keys, then two over the faces), the clusters' integer sums and representatives, the face classes, the flags and their scans.
 * Waits ONCE, to read C, V', F' and the class counts in one copy (a second time before it, only when its arrays have to grow), so it cannot be recorded
 * (WDGS_E_STATE).  colours nullable.  The mesh is read again by emit and must stay as it is until then. */
int wdgs_mesh_simplifier_count(wdgs_mesh_simplifier* simplifier, const void* vertices_f32_dev, uint32_t num_vertices, const void* faces_u32_dev, uint32_t num_faces,
                               const void* colours_rgba8_dev, const float* origin, float cell_size, uint32_t* vertices_out, uint32_t* faces_out);
/* Writes the outputs of the last count; colours_out nullable together with colours; keys_out, face_map and vertex_cluster nullable.  WDGS_E_STATE unless the last
 * count succeeded with these very vertices, faces, colours and counts; WDGS_E_CAPACITY when capacity_vertices < V' or capacity_faces < F'; nothing is written in
 * either case.  Stream-ordered, no host wait, recordable. */
int wdgs_mesh_simplifier_emit(wdgs_mesh_simplifier* simplifier, const void* vertices_f32_dev, uint32_t num_vertices, const void* faces_u32_dev, uint32_t num_faces,
                              const void* colours_rgba8_dev, void* vertices_out_f32_dev, void* colours_out_rgba8_dev, void* keys_out_u64_dev, void* faces_out_u32_dev,
                              void* face_map_u32_dev, void* vertex_cluster_u32_dev, uint32_t capacity_vertices, uint32_t capacity_faces);
/* The last count: C, the four classes of dropped faces, V' and F'; each pointer nullable.  WDGS_E_STATE when no count precedes it.  The kernels' event times are
 * the device's (wdgs_device_get_kernel_times): simplify_cell_keys, simplify_accumulate, simplify_finalize, simplify_face_keys, simplify_fold,
 * simplify_face_keys2, simplify_mark, simplify_emit_vertices, simplify_emit_faces, and the weld's and the scan's.  No device work. */
int wdgs_mesh_simplifier_stats(const wdgs_mesh_simplifier* simplifier, uint32_t* clusters, uint32_t* invalid_faces, uint32_t* outside_faces, uint32_t* collapsed_faces,
                               uint32_t* duplicate_faces, uint32_t* vertices_out, uint32_t* faces_out);

/* ---------------------------------------------------------------- Mesh adjacency, Taubin smoothing and vertex normals
 *
 * Input: an indexed mesh on the device, vertices f32[V][3], faces u32[F][3], 0 <= V < 2^31 and 0 <= 6 F < 2^32 (WDGS_E_INVALID otherwise).
 * HALF-EDGES.  Face f with corners (c0, c1, c2) is VALID when all three are < V and pairwise different; an index >= V is never used as an address.  A valid face
 * owns six slots s = 6 f + 2 j + d, j in {0, 1, 2}, d in {0, 1}: the forward slot d = 0 has the key c_j 2^32 | c_(j+1 mod 3), the backward slot d = 1 the key
 * c_(j+1 mod 3) 2^32 | c_j.  The six slots of an invalid face have the key 2^64 - 1; invalid faces are counted and contribute nothing.
 * ADJACENCY.  The distinct keys other than 2^64 - 1, ascending, are the directed edges; there are E of them, an even number.  neighbours u32[E] is their low
 * words; row_start u32[V + 1] delimits each vertex's run, ascending by construction, row_start[V] = E.  The MULTIPLICITY of the directed edge (a, b) is the number
 * of slots that carry its key, which is the number of valid faces on the undirected edge {a, b}: 1 is a BOUNDARY edge, 3 or more a NON-MANIFOLD one.  boundary
 * u32[V] is 1 on both ends of every boundary edge and 0 elsewhere.  The statistics: directed_edges = E, edges = E / 2, boundary_edges and non_manifold_edges
 * (undirected: counted where from < to), invalid_faces, boundary_vertices, isolated_vertices (empty rows), max_degree.  V - edges + (F - invalid_faces) is the
 * Euler characteristic of a mesh whose every vertex is used.
 * ONE SMOOTHING STEP step(p, w), all f32, each operation rounded once in the order written.  A vertex is copied bit for bit when it is PINNED (the flag
 * WDGS_SMOOTH_PIN_BOUNDARY is set and boundary[v] = 1) or has a non-finite coordinate.  Otherwise s = (+0, +0, +0), n = 0; for u over the row of v in ascending
 * order: skipped when p_u has a non-finite coordinate, else s += p_u per axis and n += 1.  n = 0: copied.  Else m = s / f32(n), d = m - p_v, r = p_v + w d (the
 * product, then the sum); where r has a non-finite coordinate p_v is copied instead, so the set of finite vertices never changes between steps.
 * SMOOTHING.  For `iterations` rounds: p <- step(p, lambda), then p <- step(p, mu); a step whose weight is exactly 0 is not run at all (mu = 0 is plain
 * Laplacian smoothing), iterations = 0 copies the input.  The usual Taubin pair is lambda = 0.5, mu = -0.53.  lambda and mu finite and iterations <=
 * WDGS_SMOOTH_MAX_ITERATIONS, else WDGS_E_INVALID.  Faces, colours and keys are untouched.
 * VERTEX NORMALS, area-weighted.  g_f = (p_c1 - p_c0) x (p_c2 - p_c0), each component two products and one subtraction, always from the face's own corner order
 * (every corner of a face adds the same bits).  For vertex v the slots whose key's high word is v are walked in SORTED SLOT ORDER -- ascending neighbour, then
 * ascending slot: the sort is stable -- taking the forward slots only, so that each incident valid face appears once, at f = slot / 6; g_f is added per axis
 * in that order, a g_f with a non-finite component skipped.  q = (sx sx + sy sy) + sz sz; the normal is s / sqrt(q) per axis, and (+0, +0, +0) when no face was
 * added or q is zero or not finite.
 * Every output is a function of the input alone, bit for bit, whatever the launch geometry or the order in which threads ran: one stable u64 sort of the 6 F
 * keys (the welder's), and float sums taken by one thread in an order the sort fixes.  No reference counterpart. */
#define WDGS_SMOOTH_PIN_BOUNDARY 1u
#define WDGS_SMOOTH_MAX_ITERATIONS 1024u
typedef struct wdgs_mesh_adjacency wdgs_mesh_adjacency;
int wdgs_mesh_adjacency_create(wdgs_device* dev, wdgs_mesh_adjacency** out);
int wdgs_mesh_adjacency_destroy(wdgs_mesh_adjacency* adjacency);
/* Keys, the sort, the rows, the flags and the statistics, into arrays the object owns (it grows them as needed: 44 bytes per slot -- 264 per face, the sort's pairs among them -- and 32 per vertex, the
 * smoothing steps' second position buffer f32[V][3] among them, so that smooth allocates nothing).  Waits ONCE, to read E and the statistics in one copy (a second
 * time before it, only when its arrays have to grow), so it cannot be recorded (WDGS_E_STATE).  The faces are read again by normals and must stay as they are
 * until then. */
int wdgs_mesh_adjacency_count(wdgs_mesh_adjacency* adjacency, const void* faces_u32_dev, uint32_t num_faces, uint32_t num_vertices, uint32_t* directed_edges);
/* Writes row_start_out u32[V + 1], neighbours_out u32[E] and boundary_out u32[V] of the last count, each nullable.  WDGS_E_STATE when no count precedes it;
 * WDGS_E_CAPACITY when capacity_edges < E; nothing is written in either case.  Stream-ordered, no host wait, recordable. */
int wdgs_mesh_adjacency_emit(wdgs_mesh_adjacency* adjacency, void* row_start_out_u32_dev, void* neighbours_out_u32_dev, void* boundary_out_u32_dev,
                             uint32_t capacity_edges);
/* vertices_out f32[V][3] = vertices_in smoothed over the last count's adjacency; flags: WDGS_SMOOTH_PIN_BOUNDARY or 0.  vertices_out may be vertices_in; the
 * result lands in vertices_out whatever the number of steps run.  WDGS_E_STATE unless num_vertices is the last count's V.  Stream-ordered, no host wait, no
 * allocation, recordable. */
int wdgs_mesh_adjacency_smooth(wdgs_mesh_adjacency* adjacency, const void* vertices_in_f32_dev, void* vertices_out_f32_dev, uint32_t num_vertices, uint32_t iterations,
                               float lambda, float mu, uint32_t flags);
/* normals_out f32[V][3] of vertices f32[V][3] -- any positions: the smoothed ones, say -- over the last count's sorted slots.  faces must be the very faces
 * that were counted, unchanged: WDGS_E_STATE unless the pointer and both counts are the last count's.  Stream-ordered, no host wait, recordable. */
int wdgs_mesh_adjacency_normals(wdgs_mesh_adjacency* adjacency, const void* vertices_f32_dev, const void* faces_u32_dev, uint32_t num_vertices, uint32_t num_faces,
                                void* normals_out_f32_dev);
/* The last count's statistics; each pointer nullable.  WDGS_E_STATE when no count precedes it.  The kernels' event times are the device's
 * (wdgs_device_get_kernel_times): adjacency_half_edge_keys, adjacency_fold, adjacency_edges, adjacency_rows, adjacency_emit, adjacency_copy,
 * adjacency_smooth_step, adjacency_vertex_normals, and the weld's and the scan's.  No device work. */
int wdgs_mesh_adjacency_stats(const wdgs_mesh_adjacency* adjacency, uint32_t* directed_edges, uint32_t* edges, uint32_t* boundary_edges, uint32_t* non_manifold_edges,
                              uint32_t* invalid_faces, uint32_t* boundary_vertices, uint32_t* isolated_vertices, uint32_t* max_degree);

/* ---------------------------------------------------------------- Mesh rasterization: depth, face, colour and normal images of a mesh
 *
 * Input: an indexed mesh on the device, vertices f32[V][3] (world space), faces u32[F][3], optional colours rgba8[V] (the welder's and the simplifier's layout:
 * red in the low byte), the 68-float camera block, width, height, near, cull.  WDGS_E_INVALID, with nothing written: V >= 2^31 or 3 F >= 2^32; width or height
 * outside 1 .. WDGS_MESH_RASTER_MAX_SIZE; near not positive and finite; an unknown cull; a pointer that is not 4-byte aligned (the normal image: 16).
 * VERTEX, all f32, each operation rounded once: wdgs_tsdf_volume_integrate's arithmetic, so that a mesh vertex lands where fusion sampled it.  v = view (p, 1),
 * floats 0 - 15 of the block, column-major, the products summed left to right; z = v.z; sx = (((P00 v.x) / z) / 2 + 0.5) W, sy = ((((-P11) v.y) / z) / 2 + 0.5) H,
 * P00 = block[32], P11 = block[37], W and H the width and height as floats.  The vertex is USABLE when v is finite, z >= near, sx and sy are finite and
 * |sx|, |sy| <= 16384.  Its fixed-point position is X = (i32) rint(256 sx), Y = (i32) rint(256 sy), to nearest, ties to even: 8 sub-pixel bits.
 * FACE.  Each face falls into exactly one class, tested in this order, and each class is counted: INVALID, an index >= V (never used as an address); CLIPPED, a
 * vertex that is not usable; DEGENERATE, A = 0; CULLED, dropped by cull; EMPTY, no pixel centre of the viewport inside its bounding box; RASTERIZED, the rest.
 * A = (X1 - X0)(Y2 - Y0) - (X2 - X0)(Y1 - Y0) in i64.  THERE IS NO NEAR-PLANE AND NO GUARD-BAND CLIPPING: a face with a vertex nearer than `near`, or further
 * than 16384 pixels from the origin of the image, is dropped whole.
 * cull is WDGS_CULL_NONE, WDGS_CULL_BACK (drops A > 0) or WDGS_CULL_FRONT (drops A < 0): FRONT IS A < 0.  Under the library's cameras the view matrix is a rotation
 * into +x right, +y down, +z forward, P00 > 0 and P11 < 0, so (sx, sy) is (v.x, v.y) / z scaled by positive numbers.  A face wound counter-clockwise seen from
 * outside has g = (p1 - p0) x (p2 - p0) pointing outwards, and a rotation keeps that; a camera outside the surface sees it when g . v0 < 0; and for a triangle in
 * front of the camera the sign of the area of its projection (v.x / z, v.y / z) is the sign of g . v0 (the triangle (0,0,1), (1,0,1), (0,1,1) has g = (0,0,1),
 * g . v0 = 1 and area +1).  So the faces extract_triangles winds outwards show A < 0 to a camera outside.  A camera block with P00 P11 > 0, or a view matrix
 * that mirrors, swaps the two.
 * COVERAGE, integers only.  Pixel (i, j) has the centre c = (256 i + 128, 256 j + 128).  s = sign(A); edge k runs from vertex a = k + 1 to b = k + 2 (mod 3);
 * e_k = s ((Xb - Xa)(c.y - Ya) - (Yb - Ya)(c.x - Xa)) in i64, so e_0 + e_1 + e_2 = |A|.  The pixel is covered when every e_k > 0, or e_k = 0 and the edge OWNS
 * its line: alpha > 0 or (alpha = 0 and beta > 0), alpha = -s (Yb - Ya), beta = s (Xb - Xa).  Two faces on one edge have opposite (alpha, beta) on it, so a pixel
 * centre on a shared edge or a shared vertex belongs to exactly one of them.  The bounding box: the pixels with min X <= 256 i + 128 <= max X and the same in y,
 * clamped to the viewport.
 * DEPTH, perspective-correct, f32: lambda_k = f32(e_k) / f32(|A|) (the conversions round to nearest even); w_k = 1 / z_k; q = (lambda_0 w_0 + lambda_1 w_1) +
 * lambda_2 w_2, each lambda_k w_k rounded; zp = 1 / q.  A fragment whose zp is not finite or not > 0 is skipped.
 * HIDDEN SURFACE.  Every fragment does one unsigned 64-bit atomic min of bits(zp) 2^32 | f into a u64[W H] image cleared to all ones: the nearest depth wins,
 * equal depths go to the lowest face index, and nothing depends on the order of faces, waves or launches.
 * OUTPUTS, each nullable and written only when asked for, row-major.  A pixel no fragment reached: depth 0 (the depth maps' "nothing here"), face 0xFFFFFFFF,
 * colour {0,0,0,0}, normal {0,0,0,0}.  Otherwise depth f32 = zp; face u32 = f; colour rgba8: lambda_k recomputed for that face and pixel, per channel t =
 * ((lambda_0 w_0) C_0 + (lambda_1 w_1) C_1) + (lambda_2 w_2) C_2 with C_k the vertex's byte as a float, the byte rint(min(max(t zp, 0), 255)), alpha 255 (asking
 * for it without vertex colours: WDGS_E_INVALID); normal rgba32f: the face's geometric normal in view space, g = (v1 - v0) x (v2 - v0), each component two products
 * and a subtraction, n = g / sqrt((gx gx + gy gy) + gz gz), negated where (nx v0.x + ny v0.y) + nz v0.z > 0 (wdgs_depth_to_normals' rule), {n, 1} -- or {0,0,0,0}
 * where n is zero or not finite -- which is the depth-normal image wdgs_normal_agreement and wdgs_normal_to_rgba8 take.
 * STATISTICS: the six classes, covered_pixels (those some fragment reached) and viewport_mismatch: 1 when floats 64, 65 of the camera block are not width and
 * height.  The faces are then classified all the same, but none is drawn: every output asked for is written as all-untouched and covered_pixels is 0.
 * Every output byte is a function of the input alone.  No reference counterpart.
 *
 * Faces whose bounding box is larger than WDGS_MESH_RASTER_LARGE_FACE_PIXELS pixels on either axis are drawn by another kernel (one wave per 8 x 8 pixel
 * block) than the others (one thread per face); the bytes are the same. */
#define WDGS_CULL_NONE 0u
#define WDGS_CULL_BACK 1u
#define WDGS_CULL_FRONT 2u
#define WDGS_MESH_RASTER_MAX_SIZE 8192u
#ifndef WDGS_MESH_RASTER_LARGE_FACE_PIXELS   /* (a same-box comparison builds the library with another value: csrc/Makefile, EXTRA) */
#define WDGS_MESH_RASTER_LARGE_FACE_PIXELS 8u
#endif
typedef struct wdgs_mesh_rasterizer wdgs_mesh_rasterizer;
int wdgs_mesh_rasterizer_create(wdgs_device* dev, wdgs_mesh_rasterizer** out);
int wdgs_mesh_rasterizer_destroy(wdgs_mesh_rasterizer* rasterizer);
/* Draws the mesh into arrays the object owns -- 20 bytes per vertex, 8 per face, 8 per pixel, grown as needed and reused -- and resolves them into the outputs
 * asked for.  Stream-ordered, no host wait, recordable -- except a call that has to grow the arrays: that one waits once and cannot be recorded (WDGS_E_STATE;
 * encode once eagerly with the largest sizes first).  The kernels' event times are the device's (wdgs_device_get_kernel_times): raster_vertices, raster_faces,
 * raster_blocks, raster_resolve and the scan's. */
int wdgs_mesh_rasterizer_encode(wdgs_mesh_rasterizer* rasterizer, const void* vertices_f32_dev, uint32_t num_vertices, const void* faces_u32_dev, uint32_t num_faces,
                                const void* colours_rgba8_dev, const void* camera_dev, uint32_t width, uint32_t height, float near, uint32_t cull,
                                void* depth_out_f32_dev, void* face_out_u32_dev, void* colour_out_rgba8_dev, void* normal_out_rgba32f_dev);
/* The statistics of the last encode, each pointer nullable.  Copies one block back and waits, so it cannot be recorded; WDGS_E_STATE also before any encode. */
int wdgs_mesh_rasterizer_stats(wdgs_mesh_rasterizer* rasterizer, uint32_t* invalid_faces, uint32_t* clipped_faces, uint32_t* degenerate_faces, uint32_t* culled_faces,
                               uint32_t* empty_faces, uint32_t* rasterized_faces, uint32_t* covered_pixels, uint32_t* viewport_mismatch);
/* How far two depth images f32[W H] agree.  A depth is PRESENT when it is finite and > 0; b's, when b_weight_sum (nullable) is given, only where that image's
 * value is >= min_weight_sum as well.  out u64[5] = { both, only_a, only_b: the pixels where both, a alone, b alone are present;  within: of `both`, those with
 * d = |a - b| (f32) <= threshold;  sum_q: the sum over `both` of u32(min(d / max_difference, 1) 2^24), truncating }: exact integer sums, so the result does not
 * depend on the order of anything.  The mean absolute difference, clamped at max_difference, is sum_q max_difference / 2^24 / both.  0 < threshold <=
 * max_difference, both finite, and the image size as above (WDGS_E_INVALID).  Stream-ordered, no host wait, recordable. */
int wdgs_depth_agreement(wdgs_device* dev, const void* a_f32_dev, const void* b_f32_dev, const void* b_weight_sum_f32_dev, float min_weight_sum, uint32_t width,
                         uint32_t height, float max_difference, float threshold, void* out_u64x5_dev);

/* ---------------------------------------------------------------- Per-face visibility over views, and removal of unseen faces
 *
 * Three parts: an accumulator of the rasterizer's face images into per-face counters, a rule that turns counters into keep flags, and a face filter that
 * compacts a mesh by any mask.  Integer work throughout; every output byte is a function of the inputs alone.  No reference counterpart.
 *
 * THE ACCUMULATOR holds, for a mesh of F faces (0 <= F < 2^31), counters u32[F][3] = { pixels, agreeing, views }, and four totals.  One accumulate call takes
 * one VIEW: face_image u32[W H] (what wdgs_mesh_rasterizer_encode writes), and either both or neither of mesh_depth f32[W H] (the same encode's depth image)
 * and model_depth f32[W H], with model_weight_sum f32[W H] nullable beside them.  Only counts matter, so the image is read as one row of W H pixels.  For pixel p,
 * f = face_image[p]:
 *   f < F            the pixel is COUNTED: pixels[f] += 1, counted_pixels += 1;
 *   f = 0xFFFFFFFF   the pixel is EMPTY: nothing;
 *   any other f      the pixel is FOREIGN: foreign_pixels += 1; f is never used as an address.
 * A counted pixel AGREES when both depth images are given and wdgs_depth_agreement's presence rule holds for both, in that function's f32 operations:
 * a = mesh_depth[p] finite and > 0; b = model_depth[p] finite and > 0 and, when the weight sum is given, model_weight_sum[p] >= min_weight_sum; and
 * |a - b| <= threshold, the subtraction rounded once to f32.  With both depth pointers null every counted pixel agrees.  An agreeing pixel: agreeing[f] += 1,
 * agreeing_pixels += 1.  views[f] += 1 exactly once per call in which f has at least one counted pixel; the accumulated views += 1 per call.
 * OVERFLOW IS REFUSED, NOT SATURATED: a call returns WDGS_E_CAPACITY, with nothing written, when (views accumulated so far + 1) W H >= 2^32, in host arithmetic
 * on the calls made (a recorded call counts once when recorded; stats brings the host's count up to the device's), so that no pixel count can reach 2^32.
 * WDGS_E_INVALID, with nothing written: W or H outside 1 .. WDGS_MESH_RASTER_MAX_SIZE; threshold not finite and > 0 (also in the null-depth form, which does
 * not use it); exactly one depth pointer null, or a weight sum without depths; a null face image; an image pointer that is not 16-byte aligned.  The checks
 * are made in this order, the capacity check before the face image's. */
typedef struct wdgs_face_visibility wdgs_face_visibility;
int wdgs_face_visibility_create(wdgs_device* dev, wdgs_face_visibility** out);
int wdgs_face_visibility_destroy(wdgs_face_visibility* visibility);
/* Sizes the object's arrays for num_faces faces -- 28 bytes per face, grown as needed and reused -- and zeroes them, the totals and the accumulated views.
 * Stream-ordered and recordable, except a call that has to grow the arrays: that one waits once and cannot be recorded (WDGS_E_STATE). */
int wdgs_face_visibility_reset(wdgs_face_visibility* visibility, uint32_t num_faces);
/* One view, as defined above.  Stream-ordered, no host wait, recordable (a replay is one more view).  WDGS_E_STATE before a reset.  The kernels' event times
 * are the device's (wdgs_device_get_kernel_times): face_visibility_accumulate, face_visibility_advance. */
int wdgs_face_visibility_accumulate(wdgs_face_visibility* visibility, const void* face_image_u32_dev, const void* mesh_depth_f32_dev, const void* model_depth_f32_dev,
                                    const void* model_weight_sum_f32_dev, float min_weight_sum, float threshold, uint32_t width, uint32_t height);
/* The device pointer to counters u32[F][3] (null for F = 0): the counts of every accumulate enqueued before this call, written by one launch this call
 * enqueues (the pixel and agreeing counts are kept as the halves of one 64-bit word per face, so that a run of pixels is one add), complete once the stream
 * has run and valid until the next get, reset or destroy.  Stream-ordered, no host wait, recordable.  WDGS_E_STATE before a reset. */
int wdgs_face_visibility_get(wdgs_face_visibility* visibility, void** counters_u32_dev);
/* The totals since the reset, each pointer nullable: the accumulated views, foreign_pixels, counted_pixels, agreeing_pixels.  Copies one block back and waits,
 * so it cannot be recorded (WDGS_E_STATE, also before a reset). */
int wdgs_face_visibility_stats(wdgs_face_visibility* visibility, uint64_t* views, uint64_t* foreign_pixels, uint64_t* counted_pixels, uint64_t* agreeing_pixels);
/* THE RULE.  keep u8[F]: keep[f] = 1 when pixels >= min_pixels and views >= min_views and agreeing >= min_agreeing and
 * agreeing 65536 >= min_agreeing_q16 pixels (both products in u64), else 0, for counters u32[F][3] anywhere on the device.  min_agreeing_q16 is a fraction of
 * 65536, at most 65536 (WDGS_E_INVALID; F >= 2^31 likewise); the hosts convert a fraction in [0, 1] with rint(fraction 65536).  A face with pixels = 0 passes the
 * fourth test and fails the first unless min_pixels = 0.  Stream-ordered, no host wait, recordable. */
int wdgs_face_visibility_flags(wdgs_device* dev, const void* counters_u32_dev, uint32_t num_faces, uint32_t min_pixels, uint32_t min_views, uint32_t min_agreeing,
                               uint32_t min_agreeing_q16, void* keep_u8_dev);
/* THE FILTER: wdgs_mesh_components' compaction for an arbitrary mask.  faces u32[F][3] over V vertices, 0 <= F, V < 2^31 (WDGS_E_INVALID otherwise), keep
 * u8[F] on the device.  A face is KEPT when its flag is non-zero and its three indices are < V; a vertex is kept exactly when a kept face names it.  A face
 * with an index >= V is counted in invalid_faces whatever its flag, is never kept and never read as an address. */
typedef struct wdgs_mesh_face_filter wdgs_mesh_face_filter;
int wdgs_mesh_face_filter_create(wdgs_device* dev, wdgs_mesh_face_filter** out);
int wdgs_mesh_face_filter_destroy(wdgs_mesh_face_filter* filter);
/* Flags faces and vertices into arrays the object owns (8 bytes per face and per vertex, grown as needed), scans both with the library's scan, waits and
 * returns V', F' and the invalid faces; cannot be recorded (WDGS_E_STATE).  The flags are read here only; the faces are read again by compact and must stay as
 * they are until then. */
int wdgs_mesh_face_filter_select(wdgs_mesh_face_filter* filter, const void* faces_u32_dev, uint32_t num_faces, uint32_t num_vertices, const void* keep_u8_dev,
                                 uint32_t* kept_vertices, uint32_t* kept_faces, uint32_t* invalid_faces);
/* wdgs_mesh_components_compact's signature and rules for the last select: kept faces in their original order with their indices rewritten, faces_out
 * u32[F'][3]; kept vertices in ascending original index, vertices_out f32[V'][3] gathered from vertices f32[V][3] (both nullable together); vertex_map u32[V']
 * and face_map u32[F'] (each nullable).  WDGS_E_CAPACITY, with nothing written, when capacity_vertices < V' or capacity_faces < F'; WDGS_E_STATE when no select
 * precedes it.  Stream-ordered, no host wait, recordable. */
int wdgs_mesh_face_filter_compact(wdgs_mesh_face_filter* filter, const void* vertices_f32_dev, void* vertices_out_f32_dev, void* faces_out_u32_dev,
                                  void* vertex_map_u32_dev, void* face_map_u32_dev, uint32_t capacity_vertices, uint32_t capacity_faces);

/* ---------------------------------------------------------------- Vertex colours baked from photographs
 *
 * An accumulator of views into per-vertex integer sums, and a resolve that turns the sums into rgba8 vertex colours.  Integer sums throughout, so the state
 * does not depend on the order of the views and every output byte is a function of the inputs alone.  No reference counterpart.
 *
 * STATE, for a mesh of V vertices (0 <= V < 2^31): sums u64[V][4] = { R, G, B, Wt }, one 32-byte row per vertex; views u32[V]; and six u64 totals.
 * One accumulate call takes one VIEW: vertices f32[V][3] (world space), normals f32[V][3] (nullable), the 68-float camera block, image rgba8[W H] (red in the
 * low byte, row-major; its alpha is ignored), mesh_depth f32[W H] (nullable: the depth image wdgs_mesh_rasterizer_encode wrote for this mesh and camera),
 * W, H, near, depth_tolerance, min_cos.  If floats 64 and 65 of the camera block are not W and H the call adds 1 to viewport_mismatch and nothing else.
 * Otherwise, for vertex p:
 *   1. POSITION.  The rasterizer's VERTEX rule above, verbatim: v, z, sx, sy, usable, X = (i32) rint(256 sx), Y = (i32) rint(256 sy).  A vertex that is not
 *      usable stops here; a usable one counts in `usable`.
 *   2. IN THE IMAGE.  X' = X - 128, Y' = Y - 128 (positions relative to the centre of texel (0, 0)); 0 <= X' <= 256 (W - 1) and 0 <= Y' <= 256 (H - 1), else the
 *      vertex stops; it counts in `in_image`.  i0 = X' >> 8, a = X' & 255, i1 = min(i0 + 1, W - 1); j0, b, j1 likewise from Y'.  No texel outside the image is read.
 *   3. OCCLUSION, only with mesh_depth.  Each of the four texels (i0 | i1, j0 | j1) must hold d finite and > 0 with |z - d| <= depth_tolerance, the subtraction
 *      rounded once to f32; all four, else the vertex stops: a vertex on a silhouette is skipped in that view.  A vertex that passes, and every vertex in the
 *      image when there is no depth image, counts in `visible`.
 *   4. WEIGHT.  Without normals Q = 256.  With normals n, all f32, each operation rounded once, no contraction, divide and square root correctly rounded:
 *      nv_i = (view[i] n.x + view[4 + i] n.y) + view[8 + i] n.z for i = 0, 1, 2;  dot = (nv.x v.x + nv.y v.y) + nv.z v.z;  nn = (nv.x nv.x + nv.y nv.y) + nv.z nv.z
 *      and vv likewise from v;  c = (-dot) / sqrt(nn vv).  The vertex stops when c is not finite or c < min_cos.  Q = (u32) rint(256 (c > 1 ? 1 : c)), to
 *      nearest, ties to even; the vertex stops when Q = 0.  A vertex that passes counts in `accumulated`.
 *   5. SAMPLE, integers only.  With T00, T10, T01, T11 the bytes of one channel at (i0, j0), (i1, j0), (i0, j1), (i1, j1):
 *      S = (256 - a)(256 - b) T00 + a (256 - b) T10 + (256 - a) b T01 + a b T11;  s = (S + 128) >> 8, at most 65280.
 *   6. ADD.  R += Q s_red, G += Q s_green, B += Q s_blue, Wt += Q, views = min(views + 1, 2^32 - 1).  One view adds less than 2^24 to a sum: no sum can
 *      overflow within 2^40 views.  The row is read and written by the one thread that owns the vertex, with plain loads and stores.
 * TOTALS, cumulative since the reset: usable, in_image, visible, accumulated, viewport_mismatch (calls); and baked_vertices of the last resolve.
 * RESOLVE.  A vertex is BAKED when views >= max(min_views, 1) and Wt >= max(min_weight, 1).  A baked vertex's colour: per channel the byte
 * min(255, (R + 128 Wt) / (256 Wt)), the division in u64, truncating; alpha 255.  Any other vertex gets fallback[p], or {0,0,0,0} without a fallback.
 * baked_out u8[V] (nullable) is 1 for a baked vertex and 0 for any other.
 * REFUSALS, with nothing written, tested in this order.  WDGS_E_STATE: accumulate, resolve, read or stats before a reset; num_vertices other than the reset's;
 * reset, read or stats while recording.  WDGS_E_INVALID: V >= 2^31; W or H outside 1 .. WDGS_MESH_RASTER_MAX_SIZE; near not positive and finite;
 * depth_tolerance not finite or < 0; min_cos outside [0, 1] or NaN; a null camera, image, vertices (V > 0) or colours output (V > 0); a pointer that is not
 * 4-byte aligned. */
typedef struct wdgs_mesh_colour_baker wdgs_mesh_colour_baker;
int wdgs_mesh_colour_baker_create(wdgs_device* dev, wdgs_mesh_colour_baker** out);
int wdgs_mesh_colour_baker_destroy(wdgs_mesh_colour_baker* baker);
/* Sizes the state for num_vertices vertices -- 36 bytes per vertex, grown as needed and reused -- and zeroes it and the totals.  A call that grows the arrays
 * waits once.  Cannot be recorded (WDGS_E_STATE). */
int wdgs_mesh_colour_baker_reset(wdgs_mesh_colour_baker* baker, uint32_t num_vertices);
/* One view, as defined above.  Stream-ordered, no host wait, no allocation, recordable (a replay is one more view).  The kernel's event time is the device's
 * (wdgs_device_get_kernel_times): mesh_bake_accumulate. */
int wdgs_mesh_colour_baker_accumulate(wdgs_mesh_colour_baker* baker, const void* vertices_f32_dev, const void* normals_f32_dev, uint32_t num_vertices,
                                      const void* camera_dev, const void* image_rgba8_dev, const void* mesh_depth_f32_dev, uint32_t width, uint32_t height, float near,
                                      float depth_tolerance, float min_cos);
/* colours_out rgba8[V] from the state as of this call; fallback rgba8[V] nullable and allowed to be colours_out itself; baked_out u8[V] nullable.
 * Stream-ordered, no host wait, recordable.  Kernel: mesh_bake_resolve. */
int wdgs_mesh_colour_baker_resolve(wdgs_mesh_colour_baker* baker, void* colours_out_rgba8_dev, const void* fallback_rgba8_dev, void* baked_out_u8_dev,
                                   uint32_t num_vertices, uint32_t min_views, uint64_t min_weight);
/* Copies the state to host memory, each pointer nullable: sums_out u64[V][4], views_out u32[V].  Waits, so it cannot be recorded. */
int wdgs_mesh_colour_baker_read(wdgs_mesh_colour_baker* baker, uint64_t* sums_out, uint32_t* views_out);
/* The totals, each pointer nullable.  Copies one block back and waits, so it cannot be recorded. */
int wdgs_mesh_colour_baker_stats(wdgs_mesh_colour_baker* baker, uint64_t* usable, uint64_t* in_image, uint64_t* visible, uint64_t* accumulated,
                                 uint64_t* viewport_mismatch, uint64_t* baked_vertices);

/* ---------------------------------------------------------------- A texture atlas baked from photographs
 *
 * An atlas laid out by arithmetic alone, an accumulator of views into per-texel integer sums, and a resolve that turns the sums into an rgba8 texture.
 * Integer sums throughout, so the state does not depend on the order of the views and every output byte is a function of the inputs alone.  No reference
 * counterpart.
 *
 * THE ATLAS, for a mesh of F faces (0 <= F < 2^31) and a cell edge of C texels (4, 8, 16 or 32), m = C - 3.  cells = ceil(F / 2); cell k holds faces 2k and
 * 2k + 1; cells_per_row = the least r with r r >= cells; rows = ceil(cells / cells_per_row) (0 for no cells); the atlas is Wt = cells_per_row C by Ht = rows C
 * texels, row 0 at the top, cell k at column k mod cells_per_row and row k / cells_per_row of cells.  Wt <= WDGS_MESH_TEXTURE_MAX_SIZE.
 * In a cell's own texel indices (i, j), i rightwards and j downwards: the EVEN face owns the texels with i + j <= C - 2, the ODD face those with i + j >= C,
 * nobody those with i + j = C - 1.  A texel of a face that does not exist (2k + 1 = F) is owned by nobody.  (i', j') = (i, j) for the even face and
 * (C - 1 - i, C - 1 - j) for the odd one: the face's corners v0, v1, v2 sit at the centres of the texels (i', j') = (0, 0), (m, 0), (0, m), and the corner's
 * texture coordinates, for the atlas texel (x, y) it sits on, are u = (x + 0.5) / Wt, v = 1 - (y + 0.5) / Ht (the hosts compute them).  A bilinear lookup
 * anywhere inside the triangle of those three points touches only texels the face owns.
 * STATE: rows u32[cells C C][4] = { R, G, B, Wsum }, one 16-byte row per texel in CELL-major order -- the texel (i, j) of cell k is row k C C + j C + i --
 * eleven u64 totals, and the number of accumulates since the reset.  Rows of texels nobody owns stay zero and are never read or written.
 * One accumulate call takes one VIEW: vertices f32[V][3] (world space), faces u32[F][3], the 68-float camera block, image rgba8[W H] (red in the low byte,
 * row-major; its alpha is ignored), mesh_depth f32[W H] (nullable: the depth image wdgs_mesh_rasterizer_encode wrote for this mesh and camera), W, H, near,
 * depth_tolerance, min_cos, two_sided.  If floats 64 and 65 of the camera block are not W and H the call adds 1 to viewport_mismatch and nothing else (it
 * still counts as an accumulate).  Otherwise, all f32, each operation rounded once, no contraction, divide and square root correctly rounded:
 *   1. THE FACE.  Per corner k with index a_k: P_k = the rasterizer's VERTEX rule's v (x, y) and z of vertex a_k.  The corner is GOOD when a_k < V, the three
 *      components are finite and z >= near.  A face with a corner that is not good is INVALID (a face that crosses the near plane is: nothing is clipped).
 *      n = (P1 - P0) x (P2 - P0), each component two products and a subtraction; nn = (n.x n.x + n.y n.y) + n.z n.z.  Q(p), for a point p:
 *      dot = (n.x p.x + n.y p.y) + n.z p.z;  pp = (p.x p.x + p.y p.y) + p.z p.z;  c = (-dot) / sqrt(nn pp), |c| with two_sided;  Q = 0 when c is not finite or
 *      c < min_cos, else (u32) rint(256 (c > 1 ? 1 : c)), to nearest, ties to even.  A zero-area face has Q = 0 everywhere.  A face that is not invalid is
 *      FACING AWAY when Q(P_k) = 0 at all three corners.  With the VERTEX rule's sx, sy of a corner, a face that is neither is OFF THE IMAGE when all three
 *      corners have sx < 0, or all three sx > W, or all three sy < 0, or all three sy > H.  Each face counts in at most one of invalid_faces,
 *      facing_away_faces, off_image_faces, and its texels stop here; the texels of any other face go on.
 *   2. THE TEXEL'S POINT, for every texel the face owns -- those outside the triangle included, on the face's plane extended:  u = i' / m, v = j' / m,
 *      w = (1 - u) - v;  p = (w P0 + u P1) + v P2 per component;  sx = (((P00 p.x) / p.z) 0.5 + 0.5) W and sy = ((((-P11) p.y) / p.z) 0.5 + 0.5) H as the VERTEX rule
 *      has them.  The texel is USABLE when p is finite, p.z >= near, sx and sy are finite and |sx|, |sy| <= 16384; else it stops.  X = (i32) rint(256 sx),
 *      Y likewise.  Then step 2 of the vertex colours above, verbatim: X', Y', the in-image test (`in_image`), i0, a, i1, j0, b, j1.
 *   3. OCCLUSION, only with mesh_depth: step 3 of the vertex colours, with p.z for z.  A texel that passes, and every texel in the image when there is no depth
 *      image, counts in `visible`.
 *   4. WEIGHT.  Q = Q(p); the texel stops when Q = 0, else counts in `accumulated`.
 *   5. SAMPLE, integers only: S of step 5 of the vertex colours per channel, and s = (S + 32768) >> 16, a byte.
 *   6. ADD.  R += Q s_red, G += Q s_green, B += Q s_blue, Wsum += Q.  One view adds at most 256 x 255 to a sum, so no sum can overflow within 65793 views;
 *      the accumulate that would be the 65536th since the reset is refused.  The row is read and written by the one thread that owns the texel, with one
 *      16-byte load and one 16-byte store; a texel that stopped never touches its row.
 * RESOLVE writes every texel of texture rgba8[Ht][Wt] and of state u8[Ht][Wt] (nullable).  A texel nobody owns gets 0x00000000 and state 0.  An owned texel
 * with Wsum >= max(min_weight, 1) is BAKED: per channel min((R + Wsum / 2) / Wsum, 255), integer divisions, alpha 255, state 1.  With fill != 0 an owned texel
 * that is not baked and has a baked texel among its up-to-eight neighbours in the same cell that the same face owns is FILLED: per channel (sum + n / 2) / n
 * over those n neighbours' baked bytes, alpha 255, state 2.  Any other owned texel takes the FALLBACK, alpha 255, state 0:  i'' = min(i', m),
 * j'' = min(j', m - i''), k'' = m - i'' - j'';  per channel (k'' c0 + i'' c1 + j'' c2 + m / 2) / m with c_k the byte of vertex a_k in colours rgba8[V]
 * (nullable), 0 without colours or where a_k >= V.
 * TOTALS: invalid_faces, facing_away_faces, off_image_faces, usable, in_image, visible, accumulated, cumulative over the views since the reset;
 * viewport_mismatch (calls); and baked, filled, fallback texels of the last resolve.
 * REFUSALS, with nothing written, tested in this order.  WDGS_E_INVALID at reset: F >= 2^31; C not 4, 8, 16 or 32; Wt above WDGS_MESH_TEXTURE_MAX_SIZE;
 * a starting count above 65535.  WDGS_E_STATE: layout, accumulate, resolve, read or stats before a reset; num_faces other than the reset's; the 65536th
 * accumulate; reset, read or stats while recording.  WDGS_E_INVALID: V >= 2^31; W or H outside 1 .. WDGS_MESH_RASTER_MAX_SIZE; near not positive and finite;
 * depth_tolerance not finite or < 0; min_cos outside [0, 1] or NaN; a null camera, image, faces (F > 0), vertices (F, V > 0) or texture output (F > 0); a
 * pointer that is not 4-byte aligned. */
#define WDGS_MESH_TEXTURE_MAX_SIZE 16384u
typedef struct wdgs_mesh_texture_baker wdgs_mesh_texture_baker;
int wdgs_mesh_texture_baker_create(wdgs_device* dev, wdgs_mesh_texture_baker** out);
int wdgs_mesh_texture_baker_destroy(wdgs_mesh_texture_baker* baker);
/* Sizes the state for num_faces faces in cells of `cell` texels -- 16 bytes per texel of a used cell, grown as needed and reused -- and zeroes it and the
 * totals.  `accumulates` is where the count of accumulates starts: 0, except in a test of the refusal of the 65536th.  A call that grows the array waits once.
 * Cannot be recorded (WDGS_E_STATE). */
int wdgs_mesh_texture_baker_reset(wdgs_mesh_texture_baker* baker, uint32_t num_faces, uint32_t cell, uint32_t accumulates);
/* Wt, Ht and cells_per_row of the last reset, each pointer nullable.  No device work. */
int wdgs_mesh_texture_baker_layout(wdgs_mesh_texture_baker* baker, uint32_t* width, uint32_t* height, uint32_t* cells_per_row);
/* One view, as defined above.  Stream-ordered, no host wait, no allocation, recordable (a recorded call counts once, when recorded; a replay is one more
 * view).  The count of accumulates is host arithmetic on the calls made, so REPLAYS ESCAPE THE OVERFLOW GUARD: a command buffer that holds an accumulate and is
 * submitted some 65 000 times without a reset can wrap the u32 sums silently; whoever replays one that often counts the views themselves.  The kernel's event
 * time is the device's (wdgs_device_get_kernel_times): mesh_texture_accumulate. */
int wdgs_mesh_texture_baker_accumulate(wdgs_mesh_texture_baker* baker, const void* vertices_f32_dev, uint32_t num_vertices, const void* faces_u32_dev,
                                       uint32_t num_faces, const void* camera_dev, const void* image_rgba8_dev, const void* mesh_depth_f32_dev, uint32_t width,
                                       uint32_t height, float near, float depth_tolerance, float min_cos, uint32_t two_sided);
/* texture_out rgba8[Ht Wt] and state_out u8[Ht Wt] (nullable) from the state as of this call; colours rgba8[V] nullable.  Stream-ordered, no host wait,
 * recordable.  Kernel: mesh_texture_resolve. */
int wdgs_mesh_texture_baker_resolve(wdgs_mesh_texture_baker* baker, const void* faces_u32_dev, uint32_t num_faces, uint32_t num_vertices,
                                    const void* colours_rgba8_dev, void* texture_out_rgba8_dev, void* state_out_u8_dev, uint32_t min_weight, uint32_t fill);
/* Copies the state to host memory: rows_out u32[cells C C][4] (nullable).  Waits, so it cannot be recorded. */
int wdgs_mesh_texture_baker_read(wdgs_mesh_texture_baker* baker, uint32_t* rows_out);
/* The eleven totals, in the order of TOTALS above, into totals_out u64[11].  Copies one block back and waits, so it cannot be recorded. */
int wdgs_mesh_texture_baker_stats(wdgs_mesh_texture_baker* baker, uint64_t* totals_out);

#ifdef __cplusplus
}
#endif
#endif /* WEBDGS_H */
