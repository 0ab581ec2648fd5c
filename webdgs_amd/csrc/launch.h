// The host functions one .hip file defines and another calls: the kernel launchers api.hip sequences (on dev->stream) and the scan / sort primitives the ops
// share.  Declared once, with the element types their kernels take, and included by api.hip and every defining file: a definition that drifts from its declaration
// is another overload and fails the link (-Wl,--no-undefined).  void* stops at the C ABI: api.hip casts what came in through include/webdgs.h where it hands it on.
#pragma once
#include "common.h"

struct LongWork;   // longlist.h

// ---- scan.hip
struct ScanScratch {
    DevMem<u32> block_sums;   // one sum per block of the scan, and the grand total behind them
    u32 capacity_blocks() const { return block_sums ? (u32)block_sums.count() - 1u : 0u; }
};
int scan_scratch_create(ScanScratch* s, u32 max_elements);
// Exclusive u32 scan of `count` (host-known) elements.  If total_out != nullptr, writes the grand total there.
int scan_exclusive_u32(wdgs_device* dev, ScanScratch* s, const u32* in, u32* out, u32 count, u32* total_out);
// Same, with the forward pass's stats epilogue folded into the single-block middle kernel (count must be > 0 for it to run).
// frame (nullable): the forward pass's frame number, advanced by the scan kernel -- project.hip stamps the tiles of non-finite Splats with the number
// the frame is ABOUT to get, so a stamp never has to be cleared (raster.hip compares)
// long_hdr (nullable): the header of the pass's long-list work (longlist.h), zeroed for the frame by the same kernel
struct ScanStatsEpilogue { u32* stats; u32* visible_shards; u32* host_mirror; u32 capacity; u32* frame = nullptr; u32* long_hdr = nullptr; };
int scan_exclusive_u32_stats(wdgs_device* dev, ScanScratch* s, const u32* in, u32* out, u32 count, u32* total_out, const ScanStatsEpilogue& ep);
int scan_block_sums_inplace(wdgs_device* dev, u32* block_sums, u32 num_blocks, const ScanStatsEpilogue& ep);
// scan_block_sums_inplace + the row scans of the per-workgroup tile-column counts (column_counts[columns][num_blocks] -> offsets in place, totals)
int forward_scan(wdgs_device* dev, u32* block_sums, u32 num_blocks, u32* column_counts, u32* column_totals, u32 columns, const ScanStatsEpilogue& ep);

// ---- sort.hip.  ranges: u32[segments + 1] / u32[total_tiles + 1], written; lw nullable (no long-list marks); sorted_keys: u32[*count_ptr]
int sorter_sort_segmented(wdgs_sorter* s, u32 segment_bits, u32 num_segments, u32* ranges, const LongWork* lw);
int sorter_sort_rows(wdgs_sorter* s, u32 num_tiles_x, u32 num_tiles_y, u32* ranges, const LongWork* lw);
void sorter_set_final_out_index(wdgs_sorter* s, int i);
int launch_tile_ranges(wdgs_device* dev, const u32* sorted_keys, const u32* count_ptr, u32 total_tiles, u32* ranges);

// ---- project.hip.  Per Gaussian: gaussians 6 words, sh 24 words, splats 6 words, depths / counts / offsets 1 word
// column_counts nullable (no per-column counts); dc_words nullable (SH-DC read from sh); nf_stamp u32[tiles], nf_frame one word
int launch_project_count(wdgs_device* dev, u32 n, const u32* gaussians, const u32* sh, const float* camera, const RenderSettings& st, const TileInfo& ti, u32* splats,
                         u32* depths, u32* counts, u32* visible_shards, u32* block_counts, u32* column_counts, const u32* dc_words, u32* nf_stamp, const u32* nf_frame);
// The per-view buffers of launch_project_count, for `count` views; the struct is project_count_views_kernel's argument
struct ProjectViews {
    u32 count;
    const float* camera[WDGS_MAX_BATCH_VIEWS];
    u32* splats[WDGS_MAX_BATCH_VIEWS];
    u32* depths[WDGS_MAX_BATCH_VIEWS];
    u32* tile_counts[WDGS_MAX_BATCH_VIEWS];
    u32* visible_shards[WDGS_MAX_BATCH_VIEWS];
    u32* block_counts[WDGS_MAX_BATCH_VIEWS];
    u32* column_counts[WDGS_MAX_BATCH_VIEWS];   // all null or none null
    u32* nf_stamp[WDGS_MAX_BATCH_VIEWS];        // (nullable) tiles of non-finite Splats, and each pass's frame number
    const u32* nf_frame[WDGS_MAX_BATCH_VIEWS];
};
int launch_project_count_views(wdgs_device* dev, u32 n, const u32* gaussians, const u32* sh, const RenderSettings& st, const TileInfo& ti, const ProjectViews& pv,
                               const u32* dc_words /*nullable*/);
int launch_update_stats(wdgs_device* dev, u32 n, const u32* offsets, const u32* counts, u32 capacity, u32* stats, u32* visible_shards, u32* host_mirror);
// offsets u32[n], written; block_offsets / column_offsets / column_totals: the scanned counts of project_count; keys, values: u32[capacity], written
int launch_emit_scatter(wdgs_device* dev, u32 n, const u32* splats, const u32* depths, const u32* counts, u32* offsets, const u32* block_offsets,
                        const RenderSettings& st, const TileInfo& ti, const u32* column_offsets, const u32* column_totals, u32* keys, u32* values, u32 capacity);
int launch_emit(wdgs_device* dev, u32 n, const u32* splats, const u32* depths, const u32* counts, u32* offsets, const u32* block_offsets, const RenderSettings& st,
                const TileInfo& ti, u32* keys, u32* values, u32 capacity);

// ---- raster.hip, depth.hip, contrib.hip, normal.hip: the kernels that walk the tiles' sorted entry lists (all but rasterize's walk: tilewalk.h)
// The frame the last encode composited, as its three walkers are handed it
struct CompositedFrame {
    RenderSettings st;
    TileInfo ti;
    const u32* splats;        // 6 words per Gaussian
    u32 num_splats;
    const u32* ranges;        // u32[tiles + 1]: the range table the encode used
    const u32* sorted_keys;   // u32[*count_ptr]
    const u32* sorted_vals;
    const u32* count_ptr;     // the entry count
    u32 max_batches;          // compat cap on a tile's list, in batches of 256 entries; 0 = unlimited
    const u32* nf_stamp;      // (nullable) tiles of non-finite Splats
    const u32* nf_frame;      // the frame word the stamps are compared with
};
// images are [W*H]; long_work nullable
int launch_rasterize(wdgs_device* dev, const CompositedFrame& f, u32* out_rgba8, float* out_alpha, u32* out_ncontrib, const LongWork* long_work);
// depths: the forward pass's depth words, u32[num_splats]; each of the three images nullable (that kind is not wanted)
int launch_depth_composite(wdgs_device* dev, const CompositedFrame& f, const u32* depths, float* out_weight, float* out_expected, float* out_median);
// stats: one 16-byte record { u64 sum_q; u32 max_bits; u32 pixels; } per Gaussian, added to
int launch_contribution(wdgs_device* dev, const CompositedFrame& f, void* stats);

// ---- normal.hip.  gaussians 6 words per Gaussian, camera the 68-float block; normals u32[n], written: one packed view-space normal per Gaussian
int launch_gaussian_normals(wdgs_device* dev, u32 n, const u32* gaussians, const float* camera, u32* normals);
// normals: u32[num_splats] of launch_gaussian_normals; out: rgba32f[W*H] { N.xyz, A }.  depth's walk (tilewalk.h)
int launch_normal_composite(wdgs_device* dev, const CompositedFrame& f, const u32* normals, float4* out);

// ---- tsdf.hip.  A volume of dims[0] x dims[1] x dims[2] voxels, x fastest: tsdf, weight f32 per voxel, rgb (nullable) three f32 planes
int launch_tsdf_reset(wdgs_device* dev, size_t voxels, float* tsdf, float* weight, float* rgb);
// camera the 68-float block; depth f32[W*H]; weight_sum f32[W*H] and colour rgba8[W*H] nullable
int launch_tsdf_integrate(wdgs_device* dev, const float origin[3], float voxel_size, const u32 dims[3], float truncation, float max_weight, const float* camera,
                          const float* depth, const float* weight_sum, const u32* colour, u32 width, u32 height, float min_weight_sum, float* tsdf, float* weight,
                          float* rgb);
// counts: u32 per cell, (dims[0]-1)(dims[1]-1)(dims[2]-1) of them, written
int launch_tsdf_count(wdgs_device* dev, const float origin[3], float voxel_size, const u32 dims[3], const float* tsdf, const float* weight, float min_weight, u32* counts);
// counts, offsets: launch_tsdf_count's and their scan; positions f32[total][3][3], keys u64[total][3] and colours rgba8[total][3] (both nullable; colours needs rgb)
int launch_tsdf_emit(wdgs_device* dev, const float origin[3], float voxel_size, const u32 dims[3], const float* tsdf, const float* weight, const float* rgb, float min_weight,
                     const u32* counts, const u32* offsets, float* positions, unsigned long long* keys, u32* colours);

// ---- geometry.hip.  vertices f32[V][3], faces u32[F][3]; counts u32[F], written; total: one u64, cleared and added to
int launch_sample_count(wdgs_device* dev, const float* vertices, u32 V, const u32* faces, u32 F, float density, u32 seed, u32* counts, unsigned long long* total);
// offsets: the exclusive scan of counts; points f32[total][3], face_out u32[total] (nullable)
int launch_sample_emit(wdgs_device* dev, const float* vertices, u32 V, const u32* faces, u32 F, u32 seed, const u32* offsets, u32 total, float* points, u32* face_out);
// bounds7: min x, y, z and max x, y, z of the finite points as order-preserving bit patterns, and their number
int launch_point_bounds(wdgs_device* dev, const float* points, u32 M, u32* bounds7);
// out3: u64 { n_found, n_within, sum_q }, cleared and added to
int launch_point_distance_stats(wdgs_device* dev, const float* d2, u32 K, float max_distance, float threshold, unsigned long long* out3);

// ---- meshclean.hip.  faces u32[F][3] over V vertices; every array below u32, one word per vertex, face or component
// parent[V], written: the union-find after all links (not yet flat); invalid_faces: one word, cleared and counted into
int launch_mesh_hook(wdgs_device* dev, const u32* faces, u32 F, u32 V, u32* parent, u32* invalid_faces);
// parent[V] becomes every vertex's root; used[V], written: 1 at the root of every valid face
int launch_mesh_roots(wdgs_device* dev, const u32* faces, u32 F, u32 V, u32* parent, u32* used);
// number[V]: the exclusive scan of used; vertex_component[V] and face_component[F] written; vertex_counts and triangle_counts u32[C], added to
int launch_mesh_label(wdgs_device* dev, const u32* faces, u32 F, u32 V, const u32* root, const u32* used, const u32* number, u32* vertex_component, u32* face_component,
                      u32* vertex_counts, u32* triangle_counts);
// flags[n] = keep[component[i]] (0 for an element without a component); keep u32[C]
int launch_mesh_keep_flags(wdgs_device* dev, u32 n, const u32* component, const u32* keep, u32 C, u32* flags);
// the flags of launch_mesh_keep_flags and their exclusive scans; positions f32[V][3] and positions_out (nullable together), vertex_map, face_map nullable
int launch_mesh_emit(wdgs_device* dev, const u32* faces, u32 F, u32 V, const u32* vertex_flags, const u32* vertex_offsets, const u32* face_flags, const u32* face_offsets,
                     const float* positions, float* positions_out, u32* vertex_map, u32* faces_out, u32* face_map);

// ---- meshvisibility.hip.  face_image u32[npix]; mesh_depth, model_depth (null together) and weight_sum (nullable) f32[npix], all 16-byte aligned
// pairs u64[F] (pixels | agreeing << 32), stamps u32[F], views u32[F], added to; state u64[4]: the views so far (advanced by one), foreign, counted, agreeing
int launch_face_visibility_accumulate(wdgs_device* dev, const u32* face_image, const float* mesh_depth, const float* model_depth, const float* weight_sum,
                                      float min_weight_sum, float threshold, u32 npix, u32 F, unsigned long long* pairs, u32* stamps, u32* views,
                                      unsigned long long* state);
// counters u32[F][3] = { pixels, agreeing, views }, written
int launch_face_visibility_pack(wdgs_device* dev, u32 F, const unsigned long long* pairs, const u32* views, u32* counters);
// keep u8[F], written: the rule of wdgs_face_visibility_flags
int launch_face_visibility_flags(wdgs_device* dev, u32 F, const u32* counters, u32 min_pixels, u32 min_views, u32 min_agreeing, u32 min_agreeing_q16, unsigned char* keep);
// face_flags u32[F] written; vertex_flags u32[V] cleared and set; invalid_faces: one word, cleared and counted into.  launch_mesh_emit writes the kept part
int launch_face_filter_flags(wdgs_device* dev, const u32* faces, u32 F, u32 V, const unsigned char* keep, u32* face_flags, u32* vertex_flags, u32* invalid_faces);

// ---- meshbake.hip.  vertices, normals (nullable) f32[V][3]; image rgba8[W H]; mesh_depth (nullable) f32[W H]; sums u64[V][4] = { R, G, B, Wt } in 32-byte
// aligned rows and views u32[V], added to; totals: the object's block of partial sums (meshbake.hip lays it out), added to
int launch_mesh_bake_accumulate(wdgs_device* dev, const float* vertices, const float* normals, u32 V, const float* camera, const u32* image, const float* mesh_depth,
                                u32 W, u32 H, float near, float depth_tolerance, float min_cos, unsigned long long* sums, u32* views, unsigned long long* totals);
// colours_out rgba8[V] written (fallback, nullable, may be the same array); baked_out u8[V] nullable; the baked vertices are counted into totals' second half, cleared first
int launch_mesh_bake_resolve(wdgs_device* dev, u32 V, const unsigned long long* sums, const u32* views, u32 min_views, unsigned long long min_weight, const u32* fallback,
                             u32* colours_out, unsigned char* baked_out, unsigned long long* totals);

// ---- meshtexture.hip.  cell: 4, 8, 16 or 32; vertices f32[V][3], faces u32[F][3]; image rgba8[W H]; mesh_depth (nullable) f32[W H]; rows
// u32[ceil(F / 2) cell cell][4] = { R, G, B, Wsum }, cell-major, added to; totals: the object's block of partial sums (meshtexture.hip lays it out), added to
int launch_mesh_texture_accumulate(wdgs_device* dev, u32 cell, const float* vertices, u32 V, const u32* faces, u32 F, const float* camera, const u32* image,
                                   const float* mesh_depth, u32 W, u32 H, float near, float depth_tolerance, float min_cos, u32 two_sided, u32* rows,
                                   unsigned long long* totals);
// texture_out rgba8 and state_out u8 (nullable) of cells_per_row cell by atlas_rows cell texels, every one written; colours rgba8[V] nullable; the baked, filled
// and fallback texels are counted into totals' second half, cleared first
int launch_mesh_texture_resolve(wdgs_device* dev, u32 cell, const u32* rows, const u32* faces, u32 F, u32 V, const u32* colours, u32 cells_per_row, u32 atlas_rows,
                                u32 min_weight, u32 fill, u32* texture_out, unsigned char* state_out, unsigned long long* totals);

// ---- keysort.hip: the stable u64 key sort the welder (meshweld.hip) and the simplifier (meshsimplify.hip) group by; its sizing rule: keysort_sizes.h
// The counters block, u32 words: the distinct keys, the passes run, the buffer that holds the sorted pairs, a spare, then per pass: run, input buffer, output buffer
constexpr u32 KS_C_TOTAL = 0, KS_C_PASSES = 1, KS_C_FINAL = 2, KS_C_RUN = 4, KS_C_IN = 12, KS_C_OUT = 20, KS_C_WORDS = 28;
constexpr u32 KS_PASSES = 8;   // 8-bit digits; every kernel of a pass that the plan skips returns at once
// The sort's pairs as one kernel argument.  Valid once the sort's launches are enqueued: which buffer holds the sorted order is read from the counters on the device
struct KeySortView {
    const unsigned long long* keys0;   // buffer 0: the caller's keys (never written); slot = index
    unsigned long long* keys[2];       // buffers 1 and 2: the pair buffers the passes alternate between
    u32* slots[2];
    const u32* counters;
    __device__ __forceinline__ const unsigned long long* keys_of(u32 b) const { return b == 0u ? keys0 : keys[b - 1u]; }
    __device__ __forceinline__ const u32* slots_of(u32 b) const { return b == 0u ? nullptr : slots[b - 1u]; }
    __device__ __forceinline__ const unsigned long long* sorted_keys() const { return keys_of(counters[KS_C_FINAL]); }
    __device__ __forceinline__ const u32* sorted_slots() const { return slots_of(counters[KS_C_FINAL]); }   // nullptr: slot = index (no pass ran)
};
struct KeySort {
    DevMem<unsigned long long> keys_a, keys_b;   // [n]
    DevMem<u32> slots_a, slots_b;                // [n]
    DevMem<u32> flags, ids;                      // [n]: the head flags of the sorted pairs and their scan
    DevMem<u32> table, offsets;                  // [256 * workgroups]: a pass's digit-major histogram and its scan
    DevMem<unsigned long long> or_and;           // [2 * workgroups]: the OR and the AND of every tile's keys
    DevMem<u32> counters;                        // KS_C_WORDS; the host may read TOTAL and PASSES after a wait
    ScanScratch scratch;
    u32 capacity_n = 0, capacity_table = 0, capacity_scan = 0;

    int create(wdgs_device* dev);   // the zeroed counters
    // Room for sorts of S_a and of S_b slots, grow-only; drains the lanes once before anything grows, waits for nothing otherwise
    int reserve(wdgs_device* dev, u32 S_a, u32 S_b = 0);
    // Plan, eight passes, head flags and their scan, whose total -- the number of distinct keys -- goes to total_out (device, nullable).  0 < S <= reserved
    int sort(wdgs_device* dev, const unsigned long long* keys, u32 S, u32* total_out);
    // After sort() of the same keys: rank_out[slot] = the rank of the slot's key among the distinct keys; per distinct key, at its rank: keys_out the key, and
    // gather_u32_out / gather_f32x3_out what the key's LOWEST slot has in gather_u32[S] / gather_f32x3[S][3] (each of the three nullable, a payload with its output)
    int emit(wdgs_device* dev, const unsigned long long* keys, u32 S, u32* rank_out, unsigned long long* keys_out, const u32* gather_u32, u32* gather_u32_out,
             const float* gather_f32x3, float* gather_f32x3_out);
    // sort() then emit()
    int rank(wdgs_device* dev, const unsigned long long* keys, u32 S, u32* total_out, u32* rank_out, unsigned long long* keys_out, const u32* gather_u32,
             u32* gather_u32_out, const float* gather_f32x3, float* gather_f32x3_out);
    KeySortView view(const unsigned long long* keys) const { return KeySortView{keys, {keys_a, keys_b}, {slots_a, slots_b}, counters}; }
    ScanScratch* scan() { return &scratch; }   // for the owner's further scans of at most the reserved sizes
    u32* total() const { return counters + KS_C_TOTAL; }
};

// ---- meshsimplify.hip.  vertices f32[V][3], faces u32[F][3], colours rgba8[V] (nullable); origin, inv = 1 / cell_size and cell_size: the grid (webdgs.h)
// keys u64[V], written: every vertex's cell key, 2^64 - 1 outside the grid
int launch_simplify_cell_keys(wdgs_device* dev, const float* vertices, u32 V, const float origin[3], float inv, float cell_size, unsigned long long* keys);
// rank u32[V]: the rank of every vertex's key among the distinct keys; acc u64[V][8], cleared and added to: per rank Qx, Qy, Qz, n and the four colour sums
int launch_simplify_accumulate(wdgs_device* dev, const float* vertices, const u32* colours, const u32* rank, u32 V, const float origin[3], float inv, float cell_size,
                               unsigned long long* acc);
// cluster_keys u64[totals[0]]: the distinct keys; positions f32[V][3] and colours u32[V], written at every rank whose key is a cell's
int launch_simplify_finalize(wdgs_device* dev, const unsigned long long* cluster_keys, const u32* totals, const unsigned long long* acc, u32 V, const float origin[3],
                             float inv, float cell_size, bool with_colours, float* positions, u32* colours);
// the rows of class counts (three words each) launch_simplify_face_keys leaves for F faces
u32 simplify_partial_rows(u32 F);
// keys u64[F], lead u32[F], iota u32[F], partial u32[3 rows], written: the first-stage key and smallest cluster of every candidate face, f, the class counts
int launch_simplify_face_keys(wdgs_device* dev, const u32* faces, u32 F, u32 V, const unsigned long long* vertex_keys, const u32* rank, unsigned long long* keys, u32* lead,
                              u32* iota, u32* partial);
// totals[3..5] = the folded class counts, totals[6] = 1 when the last of the totals[0] distinct keys is the outside key
int launch_simplify_fold(wdgs_device* dev, const u32* partial, u32 rows, const unsigned long long* cluster_keys, u32* totals);
// keys[f] = lead[f] * 2^32 | rank1[f] for a candidate; a dropped face keeps 2^64 - 1
int launch_simplify_face_keys2(wdgs_device* dev, const u32* lead, const u32* rank1, u32 F, unsigned long long* keys);
// rank2 u32[F]: the rank of the second key; head_face: per rank the lowest face that carries it; face_flags u32[F] written, cluster_flags u32[V] cleared and set
int launch_simplify_mark(wdgs_device* dev, const u32* faces, u32 F, u32 V, const u32* lead, const u32* rank2, const u32* head_face, const u32* rank, u32* face_flags,
                         u32* cluster_flags);
// the flags of launch_simplify_mark and their exclusive scans; colours_out (with colours), keys_out, face_map, vertex_cluster nullable
int launch_simplify_emit(wdgs_device* dev, const u32* faces, u32 F, u32 V, const u32* totals, const u32* cluster_flags, const u32* cluster_offsets,
                         const unsigned long long* cluster_keys, const float* positions, const u32* colours, const unsigned long long* vertex_keys, const u32* rank,
                         const u32* face_flags, const u32* face_offsets, float* vertices_out, u32* colours_out, unsigned long long* keys_out, u32* faces_out, u32* face_map,
                         u32* vertex_cluster);

// ---- loss.hip, dssim.hip. pred, targ: rgba8[W*H]; out: rgba32f[W*H]; acc nullable (no clear), else i32[acc_rows * 12] cleared when *acc_dirty != 0
int launch_loss_grad(wdgs_device* dev, u32 W, u32 H, const u32* pred, const u32* targ, const wdgs_training_config& cfg, float4* out, int* acc, u32 acc_rows,
                     const u32* acc_dirty);
int launch_dssim_grad(wdgs_device* dev, u32 W, u32 H, const u32* pred, const u32* targ, const wdgs_training_config& cfg, float4* out, int* acc, u32 acc_rows,
                      const u32* acc_dirty);

// ---- backward_raster.hip.  acc: i32[max(n, 1) * 12]; acc_dirty: its state word
int launch_acc_clear_if_dirty(wdgs_device* dev, int* acc, u32 n, const u32* acc_dirty);
// ranges u32[tiles + 1]; instances: the sorted indices; final_t f32[W*H], n_contrib u32[W*H], loss_grad rgba32f[W*H]; long_work nullable
int launch_backward_rasterize(wdgs_device* dev, const RenderSettings& st, u32 num_tiles_x, u32 num_tiles_y, const u32* ranges, const u32* instances, const u32* splats,
                              const float* final_t, const u32* n_contrib, const float4* loss_grad, int* acc, u32* acc_dirty, const LongWork* long_work);

// ---- backward.hip.  gradients: GaussianGradient[n], 8 words each; tile_counts u32[n]
int launch_geometry_backward(wdgs_device* dev, u32 n, const float* camera, const RenderSettings& st, const u32* gaussians, int* acc, u32* gradients);
// gradients, guard, dc_words nullable; gaussians and sh are rewritten
int launch_geometry_backward_adam(wdgs_device* dev, u32 n, const float* camera, const RenderSettings& st, u32* gaussians, int* acc, u32* acc_dirty, u32* gradients,
                                  const wdgs_adam_hyperparameters& h, const u32* tile_counts, const wdgs_optimizer_state& state, const CsView& cs, u32* sh,
                                  const u32* guard, u32* dc_words);
// sums f32[n][14], visible u32[n]; guard, overflow: one word each; mode: 1 = the step's first view (store), 2 = a later one (add)
int launch_geometry_backward_accumulate(wdgs_device* dev, u32 n, const float* camera, const RenderSettings& st, const u32* gaussians, int* acc, u32* acc_dirty,
                                        u32* gradients, float* sums, u32* visible, const u32* tile_counts, u32* guard, const u32* overflow, u32 mode);
// The per-view arguments of launch_geometry_backward_accumulate, for `count` views; the struct is geometry_backward_views_kernel's argument
struct GeometryViews {
    u32 count;
    const float* camera[WDGS_MAX_BATCH_VIEWS];
    int* acc[WDGS_MAX_BATCH_VIEWS];
    u32* acc_dirty[WDGS_MAX_BATCH_VIEWS];
    const u32* tile_counts[WDGS_MAX_BATCH_VIEWS];
    const u32* overflow[WDGS_MAX_BATCH_VIEWS];
    u32* gradients[WDGS_MAX_BATCH_VIEWS];   // nullable per view: the packed per-view GaussianGradient, for readers of getGradientsBuffer()
};
int launch_geometry_backward_views(wdgs_device* dev, u32 n, const RenderSettings& st, const u32* gaussians, const GeometryViews& gv, float* sums, u32* visible,
                                   u32* guard, u32 continues);

// ---- optimizer.hip.  guard, dc_words (u32[n][2]) and rows_out nullable; guard_seen_host: the device's pinned host_guard word
int launch_adam_repack(wdgs_device* dev, u32 n, const wdgs_adam_hyperparameters& h, const u32* tile_counts, const u32* gradients, const wdgs_optimizer_state& st,
                       const CsView& cs, u32* gaussians, u32* sh, const u32* guard, u32* dc_words);
// steps the Gaussians [first, first + count); visible: u32 per Gaussian, grad_f32: 14 floats per Gaussian
int launch_adam_repack_f32(wdgs_device* dev, u32 first, u32 count, const wdgs_adam_hyperparameters& h, const u32* visible, const float* grad_f32,
                           const wdgs_optimizer_state& st, const CsView& cs, u32* gaussians, u32* sh, const u32* guard, u32* guard_seen_host, u32* rows_out,
                           u32* dc_words);
int launch_apply_rows(wdgs_device* dev, u32 n, const u32* rows, u32 skip_first, u32 skip_count, const u32* guard, u32* guard_seen_host, u32* gaussians, u32* sh,
                      u32* dc_words);
int launch_dc_words_load(wdgs_device* dev, u32 n, const u32* sh, u32* dc_words);
int launch_dc_words_flush(wdgs_device* dev, u32 n, const u32* dc_words, u32* sh);
int launch_guard_accumulate(wdgs_device* dev, u32* flag, const u32* src, u32 overwrite);   // one word each
int launch_cs_load(wdgs_device* dev, u32 n, const wdgs_optimizer_state& st, const CsView& cs);
int launch_cs_flush(wdgs_device* dev, u32 n, const CsView& cs, const wdgs_optimizer_state& st);
// gradients: GaussianGradient[n]; acc f32[n][14], visible u32[n]
int launch_accumulate_gradients(wdgs_device* dev, u32 n, const u32* gradients, const u32* tile_counts, float* acc, u32* visible);
int launch_store_gradients(wdgs_device* dev, u32 n, const u32* gradients, const u32* tile_counts, float* acc, u32* visible);
int launch_unpack(wdgs_device* dev, u32 n, const u32* gaussians, const u32* sh, const wdgs_optimizer_state& st);

// ---- densify.hip.  rgba8 images: src sw x sh, dst dw x dh
int launch_downsample(wdgs_device* dev, const u32* src, u32 sw, u32 sh, u32* dst, u32 dw, u32 dh);
// pred, targ rgba8[W*H]; err, flags u32[W*H], written; minmax u32[2]; scratch unused
int launch_metric_map(wdgs_device* dev, u32 W, u32 H, const u32* pred, const u32* targ, float err_scale, float threshold, u32* err, u32* minmax, u32* scratch,
                      u32* flags);
// ranges u32[tiles + 1]; flags, n_contrib u32[W*H]; counts u32[num_counts], added to
int launch_metric_count(wdgs_device* dev, const RenderSettings& st, u32 ntx, u32 nty, const u32* ranges, const u32* instances, u32 num_instances, const u32* splats,
                        u32 num_splats, const u32* flags, const u32* n_contrib, u32* counts, u32 num_counts);
int launch_metric_normalize(wdgs_device* dev, u32 n, u32 divisor, u32* counts);
