// gsr_internal.h — shared between the host runtime (gsr_runtime.cpp, gsr_path.cpp, gsr_inspect.cpp,
// gsr_compat.cpp, gsr_scene.cpp, gsr_scene_save.cpp, gsr_ply.cpp) and the
// gfx950 kernels (gsr_kernels.hip, gsr_bucket_sort.hip, gsr_blend.hip, gsr_blend_derived.hip,
// gsr_scene_ops.hip, gsr_scene_densify.hip, gsr_scene_init.hip, gsr_scene_adam.hip, gsr_scene_pack.hip, gsr_image_loss.hip, gsr_project.hip, gsr_probes.hip).  Not part of the public ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <string>

#include "gsr_types.h"

struct gsr_record_grads;   // include/gsr.h
struct gsr_scene_grads;
struct gsr_densify_config;
struct gsr_init_config;

namespace gsr {

// Set the thread's last error (gsr_last_error) and return `code`.
int set_error(int code, const char* fmt, ...);


// Per-frame constants, passed by value to the kernels.
struct Frame {
    float V[16];        // view matrix (camera.cpp:53, row-major)
    float P[16];        // projection (math.cpp:91-97)
    float Rc[9];        // r_cam
    float RcT[9];       // r_cam_T
    float campos[3];
    float znear;
    float fx, fy;       // render.cu:620-621 (host-computed, shared with the oracle)
    float k;            // sigma multiplier
    int W, H;           // image size (tile_W, tile_H of the reference ABI)
    int cover_w, cover_h;   // pixels covered by the reference tile grid
    int tiles_x, tiles_y;   // internal GSR_TILE_PX tiles
};

// Radix-sort geometry.
constexpr int kSortThreads = 256;
constexpr int kSortTile = kSortThreads * 16;           // largest tile (items = 16 per thread)
constexpr int kMaxSortGroups = 8192;                    // grid upper bound (hist: 256 x this)

// Device-side frame statistics block (device memory).
struct Stats {
    unsigned long long pairs_total;   // P before the capacity clamp
    uint32_t pairs_eff;               // min(P, capacity): what sort/ranges/blend consume
    uint32_t overflow;                // bit 0: P > capacity; bit 1: the depth sort needed more
                                      // passes than were launched (depth pass budget)
    uint32_t depth_passes;            // passes the depth sort's device plan needed (binning path; 0: n/a)
    uint32_t split_unsat;             // depth split: blocks the last phase-A blend left unsaturated
                                      // (written to the host-mapped copy by the phase-B blend)
    uint32_t split_pm;                // the split point of the frame whose split_unsat that is, | the
                                      // controller's epoch << 16 (gsr_runtime.cpp split_tag)
    uint32_t spec_miss;               // depth split without phase B (speculative): a phase-A blend
                                      // left a block unsaturated, the frame is incomplete (host copy,
                                      // sticky until the host reads it)
    unsigned int bkt_over;            // bucket depth sort: items of buckets over the local capacity,
                                      // sorted through global memory (host copy, sticky diagnostics)
    unsigned int bkt_over_work;       // ... times the 8-bit passes each needed (their keys' span): the
                                      // cost of the global path (tied keys cost none; host copy, sticky)
};

// Depth split (GSR_TUNE_DEPTH_SPLIT): the frame's tiles are binned over the nearest
// part of the depth order first (phase A); its blend saves the transmittance of
// every block it leaves unsaturated, and phase B bins the rest of the depth order
// and resumes those blocks.  phase: 1 = A (save), 2 = B (resume).
// Depth split, key mode: pass 0 of a depth sort reads the whole preprocess order and
// keeps key < *kcut (mode 1, the near part: the kept count goes to *count_out and the
// threshold is copied to *kcut_copy) or key >= *kcut (mode 2, the far part, written from
// the pass's base; with sat, only items whose tile rect holds a tile phase A left
// unsaturated — the summed-area table of k_split_sat, sat_w = tiles_x + 1 — and the kept
// count goes to *count_out).  mode 0 with count: a later far pass, length *count.
struct SortFilter {
    int mode;
    const uint32_t* kcut;
    uint32_t* count_out;
    uint32_t* kcut_copy;
    const uint32_t* sat;
    int sat_w;
    const uint32_t* count;
};

// Depth split, key mode: the preprocess writes splat records only for Gaussians nearer
// than the frame's threshold (mode 1; it copies *kcut to *kcut_frame for mode 2); mode
// 2 (phase B, or a frame that ends up not split) writes only the far ones' records and
// nothing else, and returns at once when *gate is 0 (gate nullptr: always runs).
struct RecSplit {
    int mode;
    const uint32_t* kcut;
    uint32_t* kcut_frame;
    const uint32_t* gate;
};

// Depth split with a threshold partition (the near part sorted, the far part sorted
// inside phase B): cut_mode 1 = the row pass reads [0, *cut), 2 = [*cut, n); na = the
// host's split point (positions), sizes phase A's grid.
struct RowSplit {
    int cut_mode;
    uint32_t na;
    const uint32_t* cut_n;            // mode 2: the far part's kept length (a masked far sort)
};

// The next frame's depth threshold (its partition puts keys < *kcut in the near part),
// computed by phase A's blend from this frame's near depth order (gsr_blend.hip
// split_cut_update).  kcut == nullptr: no update.
struct SplitCut {
    const uint64_t* items0;
    const uint64_t* items1;
    const uint32_t* dstats;           // the near sort's pass plan (which buffer holds the result)
    const uint32_t* nnear;            // near count (nullptr: this frame sorted the whole order)
    uint32_t n, na;                   // items, the split point (positions)
    uint32_t* kcut;
};

struct BlendSplit {
    int phase;
    float* tbuf;                      // 64 floats per 8x8 block (4 blocks per tile)
    uint8_t* bflag;                   // per block: 1 = left unsaturated by phase A (tbuf valid)
    uint32_t* gate;                   // count of such blocks (cleared by phase A's row scan)
    Stats* host_st;                   // phase B publishes the count here (nullable)
    Stats* spec_host;                 // phase A with no phase B queued: an unsaturated block sets
                                      // spec_host->spec_miss (nullable)
    SplitCut cut;                     // phase A: the next frame's threshold; phase B: nnear and na only
                                      // (a near part short of the split point is tagged unmeasured)
    uint32_t pm;                      // phase B publishes it with the count (Stats::split_pm: the split
                                      // point | the controller's epoch << 16)
    uint32_t* fstatus;                // speculative phase A: an unsaturated block ors
                                      // GSR_FRAME_SPEC_MISS into the frame's validity word (nullable)
};

// ---- launch wrappers (gsr_kernels.hip; the bucket depth sort's in gsr_bucket_sort.hip, the
// blend's in gsr_blend.hip, its derived passes' in gsr_blend_derived.hip, the probes' in
// gsr_probes.hip) ----
hipError_t launch_aos_to_soa(const gsr_gaussian* aos, int64_t n, float* arrays, int64_t stride,
                             hipStream_t s);
hipError_t launch_preprocess(const float* arrays, int64_t stride, int64_t n, const Frame& fr,
                             uint4* rec, uint64_t* items, uint64_t* rect, bool packed, bool four_d, bool sh3,
                             float t, hipStream_t s, uint16_t* spans = nullptr,
                             const RecSplit* rs = nullptr);
// The same for nc = 2..kPreMultiMax cameras of one 3D scene block in one launch
// (k_preprocess_multi; gsr_render_path's frames in flight): each Gaussian is loaded once,
// its view-independent part computed once, and camera c's results go to out[c] exactly as
// launch_preprocess(fr[c], ...) writes them.  No 4D scenes, no RecSplit.
constexpr int kPreMultiMax = 4;
struct PreTargets {
    uint4* rec;
    uint64_t* items;
    uint64_t* rect;
    uint16_t* spans;   // nullable
    bool packed;
};
hipError_t launch_preprocess_multi(const float* arrays, int64_t stride, int64_t n, int nc, const Frame* const* fr,
                                   const PreTargets* out, bool sh3, hipStream_t s);
// One stable LSD pass over u64 items on bits [shift, shift + bits) (bits <= 8).
// n = n_dev ? *n_dev : n_host.  hist: 256 * groups u32, totals: 256 u32.
// ranges (nullable, final tile-sort pass): per-tile {~start, end} of key (item >> 32),
// zeroed beforehand.
// items: 8 or 16 per thread (tile = 256 * items); groups from sort_groups().
// dstats (nullable): depth-sort pass plan, zeroed per frame; pass 0 fills it,
// passes >= 1 skip themselves when they would be identities (gsr_kernels.hip).
hipError_t launch_radix_pass(const uint64_t* in, uint64_t* out, const uint32_t* n_dev, uint32_t n_host,
                             int shift, int bits, int groups, int items, uint32_t* hist, uint32_t* totals,
                             uint2* ranges, hipStream_t s, uint32_t* dstats = nullptr, int pass = 0,
                             const uint32_t* rect = nullptr, int rect_direct = 0, uint32_t* pay0 = nullptr,
                             uint32_t* pay1 = nullptr, bool rank_atomic = false,
                             const uint32_t* base_dev = nullptr, const uint32_t* gate = nullptr,
                             const SortFilter* filter = nullptr);
// Bucket depth sort (binning path; gsr_bucket_sort.hip "bucket depth sort"): the stable
// (depth key, index) order of the n items `in` (the preprocess order; rect = its packed
// tile rects by position) into items0 with the rects into pay0; items1 / pay1 are scratch.
// buckets: 256..4096 (a power of two); s_in: its buckets - 1 sorted splitters (the last
// 0xFFFFFFFF); s_out: the next frame's (quantiles of this order).  hist: groups x buckets
// u32 (groups <= kMaxBucketGroups), totals: 2 x buckets + 2 u32 (the totals, then the
// buckets' first positions and n, then a word raised when a live item has key 0xFFFFFFFF).  cap (<= kMaxBucketCap): largest bucket sorted in LDS (larger
// ones take the global path; over_host, host-mapped and nullable, counts their items, and
// over_host[1] their items times the passes they took).
constexpr int kMaxBuckets = 4096;
constexpr uint32_t kMaxBucketCap = 2048;
constexpr int kMaxBucketGroups = 512;    // chunks (workgroups) of the scatter; hist: groups x buckets
hipError_t launch_bucket_sort(const uint64_t* in, uint64_t* items0, uint64_t* items1, uint32_t n, int buckets,
                              int groups, const uint32_t* s_in, uint32_t* s_out, uint32_t* hist, uint32_t* totals,
                              const uint32_t* rect, uint32_t* pay0, uint32_t* pay1, bool rank_atomic, uint32_t cap,
                              unsigned int* over_host, hipStream_t s, int row_tiles_y, uint4* rec);
// rec: n 16-B records of scratch (the scatter's output, the local sorts' input).
// row_tiles_y > 0: the local kernel also writes the row pass's count histograms into hist
// (512 x buckets words: chunk g = bucket g, tile rows < row_tiles_y; the last bucket's chunk
// is empty unless a live item's key saturated to 0xFFFFFFFF), and the row pass then runs
// with buckets chunks, cstart = totals + buckets (the buckets' first positions) and no count
// kernel.
// Big buckets (scenes above 2M Gaussians): `buckets` must be kBigBuckets (512: ~n / 512 items
// each, sorted by one 1,024-thread workgroup in LDS, up to 16,384 items) bounded by the
// previous frame's quantiles; larger or wider-keyed buckets are sorted by launch_bucket_sort's
// local kernel in a second launch.  The scatter writes each tile in bucket order (coalesced
// 12-B records).
// groups <= kBigBucketGroups.  No fused row count.
constexpr int kBigBuckets = 512;
constexpr int kBigBucketGroups = 1024;
hipError_t launch_bucket_sort_big(const uint64_t* in, uint64_t* items0, uint64_t* items1, uint32_t n, int buckets,
                                  int groups, const uint32_t* s_in, uint32_t* s_out, uint32_t* hist, uint32_t* totals,
                                  const uint32_t* rect, uint32_t* pay0, uint32_t* pay1, bool rank_atomic, uint32_t cap,
                                  unsigned int* over_host, hipStream_t s, uint4* rec);
// Splitters for launch_bucket_sort from an order the LSD passes sorted (depth_sorted of
// items0 / items1 under dstats); live_dev (nullable): its visible count.
hipError_t launch_bkt_splitters(const uint64_t* items0, const uint64_t* items1, const uint32_t* dstats, uint32_t n,
                                const uint32_t* live_dev, int buckets, uint32_t* s_out, hipStream_t s);
// Pair emission in depth order: tile counts (gathering each Gaussian's rect
// once into srect, and zeroing the tile ranges), scan, then keys (uint16_t if
// key16 else uint32_t) + values.
hipError_t launch_emit(const uint64_t* items0, const uint64_t* items1, const uint32_t* dstats, uint32_t n,
                       const uint64_t* rect, int groups, unsigned long long* wg_scratch, Stats* stats,
                       Stats* host_mapped_stats, uint32_t pair_capacity, int tiles_x, int tiles_y, void* keys,
                       bool key16, uint32_t* vals, uint2* ranges, hipStream_t s, uint32_t* fstatus = nullptr);
// One stable key-value LSD pass of the tile sort; keys_out == nullptr marks the
// final pass (values only, tile ranges recorded).
hipError_t launch_kv_pass(const void* keys_in, const uint32_t* vals_in, void* keys_out, uint32_t* vals_out,
                          bool key16, const uint32_t* n_dev, int shift, int bits, int groups, int items,
                          uint32_t* hist, uint32_t* totals, uint2* ranges, hipStream_t s);
// One wave per 8x8 block (k_blend_w, gsr_blend.hip).  consumed: optional device counters
// (diagnostics: 16 counters, then a u64 take map entry per pixel), or with stamps the
// per-wave timeline (tools/blend_timeline.py).  band_tiles > 0: bands of that many
// tiles dealt round-robin to the XCDs; 0: one contiguous run of blocks per XCD.
// blend_exp (GSR_TUNE_BLEND_EXP): 0 gsr_blend_expf; 1 hardware exp with exact alpha tests
// and guarded transmittance tests, blocks it cannot vouch for blended again exactly;
// 2 the same with the guard band at 100 % (test hook for the exact re-blend).
hipError_t launch_blend(const uint32_t* idx, const uint2* ranges, const uint4* rec, const Frame& fr,
                        float* out, unsigned long long* consumed, bool stamps, int band_tiles, int blend_exp,
                        hipStream_t s, const BlendSplit* split = nullptr);
// Auxiliary render targets (gsr_render_aux; gsr_blend_derived.hip, like the contrib and
// backward launches below).  launch_aux_depth: z[i] = -Z of Gaussian i, the
// view-space z behind its depth key (n floats; arrays / stride / four_d / t as given to
// launch_preprocess).  launch_blend_aux (k_blend_aux): the exact blend over the same lists
// with k_blend_w's schedule, writing the colour planes (out, nullable), the accumulated
// alpha and the un-normalised depth (one plane each, nullable; depth needs z) and nfeat
// <= 8 feature planes (feat_out) composited from features (nfeat arrays of n floats); pack:
// 2 n float4 of workspace for nfeat > 4 (the features interleaved per Gaussian, k_aux_pack).
hipError_t launch_aux_depth(const float* arrays, int64_t stride, int64_t n, const Frame& fr, bool four_d, float t,
                            float* z, hipStream_t s);
hipError_t launch_blend_aux(const uint32_t* idx, const uint2* ranges, const uint4* rec, const Frame& fr,
                            float* out, float* alpha, float* depth, const float* z, const float* features,
                            int64_t n, int nfeat, float* feat_out, float4* pack, int band_tiles,
                            hipStream_t s);
// Contribution statistics (gsr_render_contrib; k_blend_contrib): the exact blend's decisions
// over the same lists with k_blend_aux's schedule, no colours.  Per Gaussian i (nullable
// each, n words, ACCUMULATED with integer atomics, one per statistic per wave and surviving
// splat): count += pixels that composited i, weight += their rint(w 2^24), wmax = max(wmax,
// float bits of w), w = fma(alpha, T, 0).  id (nullable, W*H words, overwritten): the
// composited Gaussian with the largest w per pixel, -1 for none.  overflow: the frame's
// Stats::overflow word; when it is non-zero the kernel returns without touching anything.
hipError_t launch_blend_contrib(const uint32_t* idx, const uint2* ranges, const uint4* rec, const Frame& fr,
                                uint32_t* count, unsigned long long* weight, uint32_t* wmax, int32_t* id,
                                const uint32_t* overflow, int band_tiles, hipStream_t s);
// Backward pass of the exact blend (gsr_render_backward; k_blend_backward): the same
// decisions over the same lists with k_blend_contrib's schedule, swept twice.  g_image (3 W*H
// planes) / g_alpha (W*H), at least one: the upstream gradients.  color (3 planes of n),
// opacity (n), conic (4 planes of n), center (2 planes of n), nullable each: ACCUMULATED with
// float atomics, one per component per wave and taken splat.  overflow: as above.
hipError_t launch_blend_backward(const uint32_t* idx, const uint2* ranges, const uint4* rec, const Frame& fr,
                                 const float* g_image, const float* g_alpha, float* color, float* opacity,
                                 float* conic, float* center, int64_t n, const uint32_t* overflow, int band_tiles,
                                 hipStream_t s);
// Backward pass of the exact blend with the depth and feature channels
// (gsr_render_backward_aux; k_blend_backward_aux): launch_blend_backward's with g_depth (W*H)
// and g_feat (nfeat planes of W*H) as further upstream gradients, the channels' per-Gaussian
// values (features: nfeat arrays of n; z: launch_aux_depth's output, needed with g_depth;
// pack: 2 n float4 of workspace for nfeat > 4; z and pack only when opacity, conic or center
// is wanted: nothing else reads the values) and the outputs dz (n) and feat (nfeat planes
// of n), ACCUMULATED like the others.  An output without its upstream (color without g_image,
// dz without g_depth, feat without g_feat) is not touched.  Where neither channel reaches an
// output wanted, this is launch_blend_backward itself.
hipError_t launch_blend_backward_aux(const uint32_t* idx, const uint2* ranges, const uint4* rec, const Frame& fr,
                                     const float* g_image, const float* g_alpha, const float* g_depth,
                                     const float* g_feat, const float* features, int nfeat, const float* z,
                                     float4* pack, float* color, float* opacity, float* conic, float* center,
                                     float* dz, float* feat, int64_t n, const uint32_t* overflow, int band_tiles,
                                     hipStream_t s);
// Backward pass of the projection (gsr_project_backward; k_project_backward, gsr_project.hip):
// the record gradients `in` (planes of n floats, NULL = zeros) carried on to the scene-array
// gradients `out` (ACCUMULATED, one thread per Gaussian, no atomics).  arrays / stride /
// four_d / sh3 / t as given to launch_preprocess; of fr it reads the camera, W, H and znear.
// Launch geometry from n alone; n == 0 launches nothing.  in_z (gsr_project_backward_aux, n
// floats or NULL): dL/d(-Z), an eleventh upstream entry; NULL runs the ten-entry kernel.
hipError_t launch_project_backward(const float* arrays, int64_t stride, int64_t n, const Frame& fr, bool four_d,
                                   bool sh3, float t, const gsr_record_grads& in, const gsr_scene_grads& out,
                                   hipStream_t s, const float* in_z = nullptr);
// Stable partition of the preprocess items: visible first, culled last (both in
// index order), visible count into *n_live; culled tail to out only, with dead
// rects in srect (gsr_kernels.hip "live partition").  counts: groups words.
// Depth split, phase B: summed-area table of the tiles phase A left unsaturated
// ((tiles_y + 1) x (tiles_x + 1) words), gated.
hipError_t launch_split_sat(const uint8_t* bflag, int tiles_x, int tiles_y, uint32_t* sat, const uint32_t* gate,
                            hipStream_t s);
hipError_t launch_partition(const uint64_t* in, uint32_t n, int groups, uint32_t* counts, uint32_t* n_live,
                            uint64_t* out, const uint32_t* rect, uint32_t* pay0, uint32_t* pay1, hipStream_t s);
// Tile binning (row pass + column pass, tile grids <= 256 x 256): replaces
// launch_emit + the key-value tile sort.  hist: 512 x groups; row_items /
// row_pairs: 256 each; cbins: 256 x bin_col_chunks_max(); rows_buf: pair
// capacity 8-B row items; vals/ranges as the tile sort's final pass.
hipError_t launch_bin_rows(const uint64_t* items0, const uint64_t* items1, const uint32_t* dstats, uint32_t n,
                           const uint32_t* pay0, const uint32_t* pay1, int groups, uint32_t* hist,
                           uint32_t* row_items,
                           unsigned long long* row_pairs, uint32_t pair_capacity, int tiles_y, uint64_t* rows_buf,
                           int items, hipStream_t s, const uint16_t* spans = nullptr, bool rank_atomic = false,
                           uint32_t base = 0, uint32_t* gate = nullptr, int gate_mode = 0,
                           const uint32_t* cut = nullptr, const RowSplit* rs = nullptr,
                           const uint32_t* cstart = nullptr);
hipError_t launch_bin_cols(const uint64_t* rows_buf, const uint32_t* row_items, const unsigned long long* row_pairs,
                           uint32_t* cbins, int col_groups, uint32_t pair_capacity, int tiles_x, int tiles_y,
                           uint32_t* vals, uint2* ranges, Stats* stats, Stats* host_mapped_stats, int items,
                           hipStream_t s, const uint32_t* dstats = nullptr, int passes_launched = 4,
                           bool rank_atomic = false, const uint32_t* gate = nullptr, uint32_t* fstatus = nullptr,
                           int chunk = 2048);   // row items per column-pass chunk: 1024 or 2048
uint32_t bin_col_chunks_max(uint32_t pair_capacity, int tiles_y);
// Standalone sort ABI helpers (oneSweepSort / oneSweep3DGaussianSort).
hipError_t launch_items_from_keys(const int* keys, uint32_t n, uint64_t* items, hipStream_t s);
hipError_t launch_keys_from_items(const uint64_t* items, uint32_t n, int* keys, hipStream_t s);
hipError_t launch_items_from_lwg(const gsr_lwg* rec, const uint64_t* src_perm, uint32_t n, int shift,
                                 uint32_t mask, uint64_t* items, hipStream_t s);
hipError_t launch_gather_lwg(const gsr_lwg* in, const uint64_t* stage1, const uint64_t* stage2, uint32_t n,
                             gsr_lwg* out, hipStream_t s);

// Scene editing (gsr_scene_ops.hip).  launch_mask_indices: indices[0 .. m) = the ascending i
// < n with keep[i] != 0 (three launches); counts: mask_chunks(n) + 1 words of scratch, the last
// of which receives m.  launch_gather_planes: dst[p * dst_stride + j] = src[p * src_stride +
// idx[j]] for p < nplanes, j < m, elements of 4 or 8 bytes; an index outside [0, n) reads the
// nearest valid element and counts into *bad (nullable).  scene_header (nullable): 256 bytes
// that receive a gsr_scene_header {count m, stride dst_stride, narrays nplanes}, written by
// the kernel (launched even for m == 0 when it is given).
uint32_t mask_chunks(uint32_t n);
hipError_t launch_mask_indices(const uint8_t* keep, uint32_t n, uint32_t* counts, int32_t* indices, hipStream_t s);
hipError_t launch_gather_planes(void* dst, int64_t dst_stride, const void* src, int64_t src_stride, int nplanes,
                                int elem_bytes, uint32_t n, const int32_t* idx, uint32_t m, uint32_t* bad,
                                void* scene_header, hipStream_t s);

// The scan launch of launch_mask_indices on its own (k_mask_scan, one workgroup): counts[0 ..
// chunks) become their exclusive prefix sums and counts[chunks] the total.  The densification's
// expansion scans its chunk counts with it.
hipError_t launch_scan_counts(uint32_t* counts, uint32_t chunks, hipStream_t s);

// Scene densification (include/gsr.h "scene densification"; gsr_scene_densify.hip).  The host
// has checked every argument (gsr_scene.cpp); n == 0 (m == 0, n_out == 0) launches nothing.
// launch_densify_accumulate: the statistic, one thread per Gaussian.
// launch_densify_count: per chunk of kDensifyChunk sources its output count into counts
// (densify_chunks(n) + 1 words, then scanned in place: the chunks' first output positions, and
// n_out in the last word); totals: four zeroed words that receive the sources kept, cloned,
// split and pruned (integer atomics, one per workgroup and fate).  launch_densify_emit: src[j]
// / kind[j] of every output j < n_out from the scanned counts (the sources are classified
// again: no per-source scratch).  launch_densify_split: the position and scale planes of
// the outputs of kind 2 and 3 of the new block (dst, dst_stride), from their parents in the
// source block; after the bulk move (launch_gather_planes on src).  launch_densify_gather:
// dst[p][j] = kind[j] ? 0 : src[p][idx[j]], 4-byte elements, index rule of launch_gather_planes
// for the indices it reads.  launch_reset_opacity: o = fminf(o, cap) over [0, n) of the
// block's opacity array and zeros over [0, n) of the two moment planes (nullable).
constexpr int kDensifyChunk = 1024;   // sources per workgroup of the expansion's kernels
uint32_t densify_chunks(uint32_t n);
hipError_t launch_densify_accumulate(const float* center, uint32_t n, int W, int H, float* accum, uint32_t* seen,
                                     uint32_t* bad, hipStream_t s);
hipError_t launch_densify_count(const float* arrays, int64_t stride, uint32_t n, const float* accum,
                                const uint32_t* seen, const gsr_densify_config& cfg, uint32_t* counts,
                                uint32_t* totals, hipStream_t s);
hipError_t launch_densify_emit(const float* arrays, int64_t stride, uint32_t n, const float* accum,
                               const uint32_t* seen, const gsr_densify_config& cfg, const uint32_t* offs,
                               uint32_t n_out, int32_t* src, uint8_t* kind, hipStream_t s);
hipError_t launch_densify_split(float* dst, int64_t dst_stride, uint32_t n_out, const float* arrays, int64_t stride,
                                uint32_t n, const int32_t* src, const uint8_t* kind, float shrink, uint64_t seed,
                                hipStream_t s);
hipError_t launch_densify_gather(float* dst, int64_t dst_stride, const float* src, int64_t src_stride, int nplanes,
                                 uint32_t n, const int32_t* idx, const uint8_t* kind, uint32_t m, uint32_t* bad,
                                 hipStream_t s);
hipError_t launch_reset_opacity(float* arrays, int64_t stride, uint32_t n, float cap, float* m_op, float* v_op,
                                hipStream_t s);

// Scene initialisation (include/gsr.h "scene initialisation"; gsr_scene_init.hip).  The host has
// checked every argument (gsr_scene.cpp).  launch_points_knn: the exact 3-NN statistic of n
// points into mean2, all working memory in `scratch` (knn_scratch_bytes(n) bytes: the bounds,
// two item buffers and the histograms of the sort, the sorted position planes, three box
// levels); n == 0 launches nothing.  The structure's constants, which the tests straddle: a
// leaf is kKnnLeaf consecutive points of the sorted order (one wave), a box of a coarser level
// covers kKnnFan boxes of the level below, the bounds kernel's workgroup takes kKnnBoundsChunk
// points and a sort pass's kSortTile.  launch_scene_init_fill: the header and every array of the
// new block (also for n == 0: the header alone) from the points, the colours (nullable) and
// mean2.
constexpr int kKnnLeaf = 64;
constexpr int kKnnFan = 64;
constexpr int kKnnBoundsChunk = 2048;
int64_t knn_scratch_bytes(int64_t n);
hipError_t launch_points_knn(const float* xyz, int64_t point_stride, int64_t comp_stride, uint32_t n, float* mean2,
                             uint32_t* bad, void* scratch, hipStream_t s);
hipError_t launch_scene_init_fill(void* block, int64_t stride, int narrays, const float* xyz, int64_t point_stride,
                                  int64_t comp_stride, const float* rgb, int64_t rgb_point_stride,
                                  int64_t rgb_comp_stride, uint32_t n, const float* mean2, const gsr_init_config& cfg,
                                  hipStream_t s);

// Scene optimisation (gsr_scene_adam_step; k_scene_adam, gsr_scene_adam.hip): one launch steps
// every active plane.  The plane table travels in the kernel arguments (the call never
// allocates): per active plane the block array it steps, its gradient and moment planes, its
// learning rate and how the stored value is stepped.  flags: GSR_ADAM_*; the host has
// checked every argument (gsr_scene.cpp).  n == 0 or no plane launches nothing.
enum { kAdamPlain = 0, kAdamExp = 1, kAdamOpacity = 2 };   // x - d | x exp(-d) | the logit step
struct AdamPlane {
    float* g;
    float* m;
    float* v;
    float lr;
    uint16_t array;   // index of the block array
    uint16_t kind;    // kAdam*
};
struct AdamLaunch {
    AdamPlane plane[GSR_SCENE_SH3_NARRAYS];   // the largest block kind
    int nplanes;
    float beta1, beta2, omb1, omb2, bc1, bc2, eps;
    int flags;
};
hipError_t launch_scene_adam(float* arrays, int64_t stride, uint32_t n, const AdamLaunch& L, uint32_t* bad,
                             hipStream_t s);

// Scene export (include/gsr.h "scene export").  pack_map: the row format of a block kind as
// a table, property p of a row <- block array array[p] under kind[p]; the host writer
// (gsr_ply.cpp) and the pack kernel (gsr_scene_pack.hip) walk the same table.  nprops is 0
// for a narrays that is no block kind.
enum { kPackCopy = 0, kPackLog = 1, kPackLogit = 2, kPackZero = 3 };   // bits | gsr_raw_log | gsr_raw_logit | +0
constexpr int kPackMaxProps = 73;
struct PackMap {
    uint8_t array[kPackMaxProps];
    uint8_t kind[kPackMaxProps];
    int nprops;
};
inline PackMap pack_map(int narrays) {
    PackMap m{};
    const bool four_d = narrays == GSR_SCENE4D_NARRAYS, sh3 = narrays == GSR_SCENE_SH3_NARRAYS;
    if (narrays != GSR_SCENE_NARRAYS && !four_d && !sh3) return m;
    int p = 0;
    auto put = [&](int array, int kind) {
        m.array[p] = (uint8_t)array;
        m.kind[p++] = (uint8_t)kind;
    };
    for (int c = 0; c < 3; c++) put(GSR_A_X + c, kPackCopy);
    for (int c = 0; c < 3; c++) put(0, kPackZero);   // nx ny nz
    for (int c = 0; c < 3; c++) put(GSR_A_SH0 + c, kPackCopy);
    for (int j = 0; j < 45; j++) {
        if (sh3) put(GSR_A_SH0 + 3 * (1 + j % 15) + j / 15, kPackCopy);   // channel-major f_rest <- sh[3k + c]
        else if (j < 24) put(GSR_A_SH0 + 3 + j, kPackCopy);
        else put(0, kPackZero);   // f_rest_24..44: the block never held them
    }
    put(GSR_A_OPACITY, kPackLogit);
    for (int c = 0; c < 3; c++) put(GSR_A_SCALE0 + c, kPackLog);
    for (int c = 0; c < 4; c++) put(GSR_A_ROT0 + c, kPackCopy);
    if (four_d) {
        put(GSR_A_TCENTER, kPackCopy);
        put(GSR_A_TSCALE, kPackLog);
        for (int c = 0; c < 9; c++) put(GSR_A_MOTION0 + c, kPackCopy);
    }
    m.nprops = p;
    return m;
}
// The pack kernel (k_scene_pack): rows [first, first + count) of the block's arrays as count *
// nprops contiguous floats at `rows`, one workgroup per tile of kPackTileRows rows counted from
// `first`.  The host has checked every argument (gsr_scene_save.cpp); count == 0 launches nothing.
constexpr int kPackTileRows = 64;
hipError_t launch_scene_pack(const float* arrays, int64_t stride, int narrays, uint32_t first, uint32_t count,
                             float* rows, hipStream_t s);

// The file side of both PLY writers (gsr_ply.cpp): the synthetic writers' header for n rows,
// then whatever write() appends, in a temporary file beside `path` that commit() renames over
// it.  Destroyed without a commit, it removes the temporary file and leaves `path` as it was.
// Every failure returns GSR_E_IO with the message set (`who` names the call).
class PlyFile {
public:
    PlyFile() = default;
    PlyFile(const PlyFile&) = delete;
    PlyFile& operator=(const PlyFile&) = delete;
    ~PlyFile();
    int open(const char* path, int64_t n, bool four_d, const char* who);
    int write(const void* data, size_t bytes);
    int commit();

private:
    int fd_ = -1;
    std::string path_, tmp_;
    const char* who_ = "";
};

// Image loss (gsr_image_loss; gsr_image_loss.hip): a tiled forward launch, a one-workgroup sum
// of the loss values (only with `loss`) and a tiled backward launch (only with `grad`).
// scratch, in floats: kLossSlotFloats of per-workgroup {sum |d|, sum d^2, sum SSIM} (the tiled
// launches run at most kLossMaxGroups workgroups, each walking tiles), then, only with `grad`,
// the three partial maps of 3 * W * H each.  The host has checked every argument, the scratch
// size among them (gsr_scene.cpp); c_* are grad_scale * weight / (3 W H), signed and doubled
// as the backward kernel adds them.
constexpr int kLossMaxGroups = 2048;   // 8 workgroups of 256 threads for each of 256 CUs
constexpr int64_t kLossSlotFloats = 3 * (int64_t)kLossMaxGroups;
struct LossLaunch {
    double w_l1, w_l2, w_dssim;
    float c_l1, c_l2, c_ssim;
};
hipError_t launch_image_loss(const float* x, const float* y, int W, int H, const LossLaunch& L, float* grad,
                             float* loss, float* scratch, hipStream_t s);

// Device self-check of the lane order of same-address returning LDS atomics (the
// RA rank path): runs k_rank_order_check synchronously on the current device and
// returns the lane-operations checked and how many returned a value out of lane order.
hipError_t rank_order_check(unsigned long long* lane_ops, unsigned long long* mismatches);

// Device math probe for the detmath GPU parity test.
hipError_t launch_math_probe(const float* in, int n, float* out, hipStream_t s);
// (gsr_blend.hip: the probe of the blend's own exp functions)
hipError_t launch_exp_probe(uint32_t key_lo, uint32_t key_hi, float x_big, unsigned long long* viol, uint32_t* errs,
                            hipStream_t s);
hipError_t launch_xs_probe(const float* op, int n, float* out, hipStream_t s);

// Drop-in frame into a device image on the drop-in context (gsr_compat.cpp);
// callers hold dropin_mutex().  `what` names the failing step for the message.
int dropin_render_device(gsr_gaussian* d_gaussians, int num_gaussians, const gsr_camera& cam, int num_tile_y,
                         int num_tile_x, int width_stride, int height_stride, int W, int H, float k,
                         float* d_out, const char** what);
std::mutex& dropin_mutex();
const char* last_error();   // the thread's message, as gsr_last_error reads it (gsr_runtime.cpp)

}  // namespace gsr
