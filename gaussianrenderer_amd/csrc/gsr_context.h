// gsr_context.h — the runtime context and the few internals that cross its files.  Private to
// the host files that work on a context: gsr_runtime.cpp (the workspace and the frame pipeline),
// gsr_path.cpp (the frames in flight) and gsr_inspect.cpp (readback, timing, tuning).  The files
// that need no context (gsr_camera.cpp, gsr_compat.cpp, gsr_scene.cpp) do not include it.
#pragma once

#include <mutex>
#include <vector>

#include "gsr_host.h"

namespace gsr {

// Everything that selects kernels or schedules (all settings are bit-identical): what a lane
// of gsr_render_path inherits from lane 0 (copy_settings).
struct Settings {
    int tile_items = 16;             // tile sort: items per thread (8 | 16)
    int depth_items = 0;             // depth sort: items per thread (0 = by size | 8 | 16)
    int tile_groups = 1024;          // tile sort: workgroup cap (measured best: 2 tiles of items per group)
    int tile_split_even = 1;         // tile sort: digits split evenly over the passes
    int depth_skip = 1;              // depth sort: skip trailing identity passes (device-side plan)
    int depth_compact = 2;           // live partition before the depth sort: 0 off, 1 on, 2 4D scenes only
    int depth_groups = 0;            // depth sort: workgroup cap (0 = default)
    int tile_binning = 1;            // row + column binning instead of emit + tile sort (grids <= 256 x 256)
    int bin_row_items = 4;           // binning: items per thread of a row-pass tile (4 | 8 | 16)
    int bin_col_items = 8;           // binning: items per thread of a column-pass tile (4 | 8 | 16)
    int tile_spans = 2;              // binning: drop the tiles of a splat's first four tile rows that
                                     // it provably cannot composite on (GSR_TUNE_TILE_SPANS): 0 off,
                                     // 1 on, 2 on up to kSpansAutoMax Gaussians
    int bin_col_groups = 0;          // binning: column-pass workgroups (chunks are strided over them);
                                     // 0 = by scene size (n / 1024 clamped to 1024..4096)
    int blend_exp = 1;               // blend: 1 = fast exp, exact decisions (default); 0 = gsr_blend_expf (bit-exact)
                                     // tests and guarded T tests (re-blends what it cannot vouch for)
    int depth_split = 2;             // GSR_TUNE_DEPTH_SPLIT: 0 off, 1 on, 2 on above kLargeScene Gaussians
    int blend_band_tiles = 4;        // blend: tiles per spatial band, bands dealt round-robin to the
                                     // XCDs (0: one contiguous band per XCD)
    int completion_events = 1;       // 0: no completion event / overflow query (stream capture)
    int rank_atomic = -1;            // GSR_TUNE_RANK_ATOMIC: 1 = ranks from returning LDS atomics when the
                                     // device self-check passed, 0 = ballot matching; -1 = not yet set
                                     // (the environment's GSR_RANK_ATOMIC=0 selects 0, else 1)
    // bucket depth sort (GSR_TUNE_DEPTH_BUCKETS, gsr_bucket_sort.hip "bucket depth sort")
    int fuse_rows = 1;               // GSR_TUNE_BUCKET_ROWS: the bucket sort's local kernel counts the row pass
    int col_chunk = 0;               // GSR_TUNE_COL_CHUNK: 0 = by scene size (col_chunk_for), 1024, 2048
    int bucket_sort = 1;             // 0 = LSD passes; 1 = bucket sort after the context's first frame
                                     // (big buckets above 2M, bkt_big); 2 = test hook: as 1 with a local
                                     // capacity of 64 items (most buckets take the global path); 3 = the
                                     // small-bucket kind at any size (A/B)
};

// The depth split's controller: what check_overflow and the preprocess adapt from frame to
// frame.  An aux frame takes no part in it (aux_frame_locked saves and restores it).
struct SplitCtl {
    int split_pm = 250;              // split point: phase A bins the nearest split_pm / 1000 of the depth order
    uint32_t split_epoch = 0;        // bumped at every restart of the controller (retry, knob): phase B
                                     // publishes it with the split point, so evidence from before the
                                     // restart is never taken for the restarted split point's
    int split_floor = 0;             // 5/4 of the last split point that left blocks unsaturated
    int split_clean = 0;             // checked split frames in a row that left none
    int split_off_frames = 0;        // frames since the split point reached 1000 (split off); after
                                     // split_retry of them, on a new camera, the split is tried again
    int split_retry = 0;             // frames before the next retry (kSplitRetry, doubling after each
                                     // retry that found no saturating view, back after a clean one)
    float split_off_view[32] = {};   // V and P of the frame the split was turned off on
    float prev_view[32] = {};        // V and P of the previous frame (a still camera: the same twice)
    bool split_seen = false;         // a split frame was blended since the last controller update
    bool split_spec = false;         // speculate: queue no phase B (the split point cannot shrink further
                                     // and 8 checked frames in a row needed none); a frame that then
                                     // leaves a block unsaturated is reported as GSR_E_OVERFLOW
    float split_view[32] = {};       // V and P of this context's last split frame: a frame speculates
                                     // only with the same camera (its threshold then fits it)
    bool split_key_ready = false;    // *kcut holds a threshold from an earlier split frame of this context
};

struct FrameEvents {
    int mode;
    hipEvent_t ev[GSR_NUM_STAGES + 1];
};

}  // namespace gsr

struct gsr_context {
    std::mutex mu;
    // capacities (elements) that size several buffers each; a buffer with a size of its own
    // knows it (DevBuf::capacity)
    int64_t n_cap = 0, p_cap = 0;
    DevBuf<uint4> rec;
    DevBuf<uint64_t> items[2];
    // pair buffers: p_cap u64 each, used as {keys: p_cap x 4 B, values: p_cap x 4 B}
    DevBuf<uint64_t> pairs[2];
    DevBuf<uint64_t> rect;           // per-Gaussian tile rectangle (preprocess output)
    bool rect_packed = false;        // this frame's rects are packed (binning path, set by gsr_preprocess)
    DevBuf<uint64_t> srect;          // binning path: two u32 rect-payload buffers the depth sort carries
                                     // (pack_rect), one of them depth-ordered at its end
    DevBuf<uint16_t> spans;          // binning path: per-Gaussian tile row spans (tile_row_spans)
    bool spans_frame = false;        // this frame's preprocess wrote them (the row pass reads them)
    DevBuf<uint32_t> hist;
    DevBuf<uint32_t> totals;
    DevBuf<unsigned long long> wg;
    DevBuf<gsr::Stats> stats;             // device: [0] frame, [1] sticky
    gsr::Stats* hstats = nullptr;         // host-mapped copy of the sticky stats
    gsr::Stats* hstats_dev = nullptr;
    DevBuf<uint2> ranges;
    DevBuf<float> soa_tmp;
    DevBuf<unsigned long long> consumed; // diagnostics: blend counters (or stamps)
    bool diagnostics = false;
    int blend_variant = 0;
    float time = 0.0f;               // frame time for 4D scene blocks
    gsr::Settings set;                    // the knobs a lane inherits; the knob-backed fields outside it (blend_variant,
                                     // diagnostics, timing, fail_frame, path_shared_pre, inflight, time) are lane 0's
    gsr::SplitCtl ctl;                    // the depth split's controller (a lane gets split_pm at creation and by its knob)
    int depth_budget = 4;            // binning path: depth passes launched (adapts to the plan's needs)
    int depth_budget_streak = 0;     // consecutive checked frames that needed fewer passes than the budget
    int depth_budget_seen = 0;       // most passes any of those frames needed
    int passes_launched = 4;         // passes the last depth sort launched
    DevBuf<uint32_t> dstats;         // depth-sort pass plan: 4 final words + 4 per upsweep workgroup
    DevBuf<uint32_t> nlive;          // visible count of the live partition (device word)
    bool compact_frame = false;      // this frame's preprocess items went to items[1] for the partition
    bool last_compact = false;       // the last sorted frame sorted only its visible prefix
    DevBuf<uint64_t> binmeta;        // binning: row pair totals (u64 x 256) then row item totals (u32 x 256)
    DevBuf<uint32_t> cbins;          // binning: column counts per chunk (256 x chunks)
    bool last_binned = false;        // the last sorted frame took the binning path
    bool split_frame = false;        // the sorted frame is split (phase A lists binned by sort_locked)
    bool split_rebin = false;        // phase B's lists replaced phase A's: a repeated blend bins phase A again
    bool frame_spec = false;         // the sorted frame is blended without phase B
    uint32_t split_na = 0;           // phase A's depth-order prefix (count mode) / the split point
    bool split_key = false;          // the preprocess left its items in items[1] for a threshold partition
    bool frame_key = false;          // the sorted frame is split in key mode (near part sorted, far part
                                     // sorted by phase B)
    bool last_split_key = false;     // the last sorted frame left its far part unsorted (phase B may not run)
    DevBuf<uint32_t> kcut;           // depth split: the next frame's depth threshold (device word)
    DevBuf<uint32_t> kcut_frame;     // depth split: this frame's threshold (the near sort copies it)
    DevBuf<uint64_t> src_items;      // depth split, key mode: the preprocess order (both sorts' pass 0 read it)
    DevBuf<uint32_t> sat;            // depth split, phase B: summed-area table of the unsaturated tiles
    DevBuf<uint32_t> nfar;           // depth split, phase B: far items whose rect touches one (device word)
    uint64_t* pre_out = nullptr;     // where the preprocess wrote its items
    bool records_partial = false;    // the preprocess wrote only the near Gaussians' records
    const float* pre_arrays = nullptr;   // the preprocessed scene arrays (the far record pass re-reads them)
    const void* pre_scene = nullptr;     // the scene pointer gsr_preprocess was given
    int64_t pre_stride = 0;
    int pre_layout = 0;
    DevBuf<uint32_t> dstats_far;     // depth split: the far sort's pass plan
    int far_launched = 4;            // passes the far sort launched
    DevBuf<float> tbuf;              // depth split: saved transmittance, 64 floats per 8x8 block
    DevBuf<uint8_t> bflag;           // depth split: per block, left unsaturated by phase A
    DevBuf<uint32_t> gate;           // depth split: count of such blocks (device word)
    int64_t split_cap = 0;           // blocks tbuf / bflag hold
    bool rank_ok = false;            // the device passed the rank-order self-check (ensure_static)
    bool overflow_seen = false;      // an overflow was reported since the last gsr_sync (which reports it again)
    // bucket depth sort
    DevBuf<uint32_t> bkt_split;      // 2 x kMaxBuckets splitters (double-buffered: read one, write the other)
    DevBuf<uint4> bkt_rec;           // the scatter's 16-B records (n_cap of them, with the items)
    int bkt_par = 0;                 // the half the next bucket-sorted frame reads
    int bkt_B = 0;                   // buckets the splitters were made for (0: none yet)
    const void* bkt_scene = nullptr; // the scene they were made from (another scene reseeds them)
    unsigned int bkt_work_seen = 0;  // hstats->bkt_over_work when the last frame was prepared
    bool bds_frame = false;          // this frame's preprocess items went to items[1] for the bucket sort
    bool last_bds = false;           // the last sorted frame was bucket-sorted (order in items[0], no pass plan)
    bool bkt_rows_fused = false;     // its local sorts wrote the row pass's counts (bucket = row chunk): the
                                     // next binning skips its count kernel (once: the row scan consumes them)
    int split_state_hold = -1;       // >= 0: the sorted frame is an aux frame (gsr_render_aux), and
                                     // GSR_TUNE_DEPTH_SPLIT_STATE reads this, the state of the frame before it
    DevBuf<float> aux_z;             // gsr_render_aux: -Z per Gaussian (the depth channel's values)
    DevBuf<float> rec_grads;         // gsr_render_backward_scene without a caller's scratch: ten planes of n floats (_aux: eleven)
    DevBuf<float4> aux_pack;         // gsr_render_aux, nfeat > 4: the features interleaved per Gaussian
    int fail_frame = 0;              // GSR_TUNE_FAIL_FRAME: gsr_render_path fails this frame (> 0) once
    uint32_t* fstatus = nullptr;     // the current frame's validity word (gsr_render_path_status; device,
                                     // nullable): GSR_FRAME_* bits, written by its column scans / blend
    // frame state
    gsr::Frame fr{};
    int64_t n = 0;
    bool have_pre = false, have_sort = false;
    int pair_buf = 0;
    int ntiles = 0;
    hipStream_t stream = nullptr;
    hipEvent_t done_ev = nullptr;
    bool pending = false;
    // timing
    int timing = 0;
    int timing_stride = 1;           // record the timing events on every k-th frame only
    int64_t timing_count = 0;        // frames seen since timing was enabled
    bool timing_now = false;         // this frame records events
    std::vector<hipEvent_t> ev_pool;
    std::vector<gsr::FrameEvents> ev_frames;
    gsr::FrameEvents cur{};
    // frames in flight (gsr_render_path): lane 0 is this context on the caller's
    // stream; lane l >= 1 is a private child context (own workspace) on its own
    // non-blocking stream.  Children are only touched under this context's mutex.
    int inflight = 3;
    std::vector<gsr_context*> lanes;          // lanes[l - 1] = child of lane l
    std::vector<hipStream_t> lane_streams;    // lane_streams[l - 1]
    // shared preprocess (GSR_TUNE_PATH_SHARED_PRE): one k_preprocess_multi launch on lane 0's
    // stream writes the preprocess outputs of every lane's frame of a group.  Each lane
    // holds a second set of those outputs (alt_*, alt_cap Gaussians): the launch writes
    // the set the lane's previous frames are not using, which becomes the lane's current
    // set (switch_pre_set); alt_ev, on the lane's stream, marks the end of the work that
    // used the other one.
    int path_shared_pre = 1;
    int64_t shared_launches = 0;     // GSR_TUNE_PATH_SHARED_LAUNCHES (lane 0 counts)
    DevBuf<uint4> alt_rec;
    DevBuf<uint64_t> alt_items;
    DevBuf<uint64_t> alt_rect;
    DevBuf<uint16_t> alt_spans;
    int64_t alt_cap = 0;
    hipEvent_t alt_ev = nullptr;
    hipEvent_t pre_ev = nullptr;     // lane 0: after a group's shared launches
    hipEvent_t fork_ev = nullptr;
    std::vector<hipEvent_t> join_evs;         // one per child lane
    std::vector<hipEvent_t> alias_evs;        // ring of `inflight` events: output reuse across lanes
};

// every function declared from here on is internal to libgsr.so: hidden, or each would be one
// more exported symbol
#pragma GCC visibility push(hidden)

namespace gsr {

// Scenes above this many Gaussians: tile row spans off (their by-index code gather
// leaves the L2), the depth split on (GSR_TUNE_TILE_SPANS / GSR_TUNE_DEPTH_SPLIT = 2).
constexpr int64_t kLargeScene = 3 << 19;

// GSR_TUNE_DEPTH_SPLIT asks for the depth split on a frame of n Gaussians.
inline bool split_wanted(const gsr_context* c, int64_t n) {
    return c->set.depth_split == 1 || (c->set.depth_split == 2 && n > kLargeScene);
}

// The depth split applies to this context's frames of n Gaussians (binning path;
// gsr_render / gsr_render_path decide it per frame, the stage API never).  Its two blend
// phases always run the exact blend, whatever GSR_TUNE_BLEND_EXP says for other frames.
inline bool split_enabled(const gsr_context* c, int64_t n) {
    return n > 0 && c->blend_variant != 3 && c->ctl.split_pm < 1000 && split_wanted(c, n);
}

// GSR_TUNE_DEPTH_SPLIT_STATE: how the last sorted frame ran (aux frames do not count).
inline int split_state(const gsr_context* c) {
    if (c->split_state_hold >= 0) return c->split_state_hold;
    return !c->split_frame ? 0 : !c->frame_key ? 1 : c->frame_spec ? 3 : 2;
}

// The split controller starts again from split point pm (the retry after a turn-off, the
// GSR_TUNE_DEPTH_SPLIT_PERMILLE knob): a new epoch, no floor, no clean frames, no threshold.
inline void split_restart(gsr_context* c, int pm) {
    c->ctl.split_pm = pm;
    c->ctl.split_epoch++;
    c->ctl.split_floor = 0;
    c->ctl.split_clean = 0;
    c->ctl.split_key_ready = false;
}

// The values half of pair buffer b (the keys are the first p_cap words).
inline uint32_t* pair_vals(gsr_context* c, int b) { return reinterpret_cast<uint32_t*>(c->pairs[b].get()) + c->p_cap; }

// ---- gsr_runtime.cpp: what gsr_path.cpp and gsr_inspect.cpp call.  The _locked functions
// are called with the context's mutex held.

// The rank-order self-check's result for the current device (run once per process and device).
struct RankCheck {
    int state = -1;                  // -1 not run, 0 failed / not gfx950, 1 passed
    unsigned long long ops = 0, bad = 0;
};
int rank_check_device(RankCheck* out);
int default_rank_atomic();           // GSR_TUNE_RANK_ATOMIC before it is set: the environment's

// the workspace: the fixed-size buffers, the per-Gaussian buffers, the pair buffers
int ensure_static(gsr_context* c);
int ensure_n(gsr_context* c, int64_t n);
int ensure_pairs(gsr_context* c, int64_t p);

// A frame's preprocess: the host-side plan, its launch on stream s (or, for a shared launch
// that wrote the planned outputs, the note that it is queued); preprocess_locked is plan + launch.
int preprocess_plan(gsr_context* c, const void* scene, int layout, int64_t n, const gsr_camera* cam, int W, int H,
                    int nx, int ny, int ws, int hs, float k, void* stream);
int preprocess_launch(gsr_context* c, hipStream_t s);
void preprocess_queued(gsr_context* c);
int preprocess_locked(gsr_context* c, const void* scene, int layout, int64_t n, const gsr_camera* cam, int W, int H,
                      int nx, int ny, int ws, int hs, float k, void* stream);
int sort_locked(gsr_context* c, bool allow_split);
int blend_locked(gsr_context* c, float* d_out);
int far_records_locked(gsr_context* c, bool gated);

}  // namespace gsr

#pragma GCC visibility pop
