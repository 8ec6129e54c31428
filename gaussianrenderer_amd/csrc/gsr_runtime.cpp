// gsr_runtime.cpp — the context and its frame pipeline, behind the C ABI of include/gsr.h.
//
// Owns the persistent per-context workspace (sized by high-water mark, never
// allocated per frame — the reference does ~10 cudaMalloc/cudaFree per frame,
// render.cu:891-902, 1144-1156) and orchestrates the stage kernels on one HIP
// stream: the stage API, gsr_render, the auxiliary, contribution and backward frames.
// Around it: gsr_path.cpp (frames in flight), gsr_inspect.cpp (readback, timing, tuning,
// device probes), gsr_compat.cpp (the reference viewer's drop-in entry points),
// gsr_camera.cpp (the camera helpers) and gsr_scene.cpp (the context-free scene API).
// The context and what crosses these files is gsr_context.h.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include <hip/hip_runtime.h>

#include "gsr_context.h"

using namespace gsr;

// ------------------------------------------------------------------ errors

static thread_local std::string g_err;

namespace gsr {
int set_error(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
const char* last_error() { return g_err.c_str(); }
}  // namespace gsr

extern "C" const char* gsr_last_error(void) { return g_err.c_str(); }
extern "C" const char* gsr_version(void) { return "gsr 0.1 (gfx950)"; }

extern "C" int gsr_device_available(void) {
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) return 0;
    return c > 0 ? 1 : 0;
}

// ------------------------------------------------------------------ workspace, split controller

namespace {

constexpr int kSplitMinPm = 20;       // smallest split point (per mille)
constexpr int kSplitRetry = 256;      // frames with the split turned off before it is tried again
constexpr int kSplitRetryMax = 1 << 14;

// Buckets of the bucket depth sort for n items: about 1,024 items per bucket (local sorts
// of ~930 live items at config 2 against a 2,048-item capacity), 256..kMaxBuckets.
int bkt_count(int64_t n) {
    int b = 256;
    while (b < gsr::kMaxBuckets && (int64_t)b * 1024 < n) b *= 2;
    return b;
}

// Two kinds of bucket sort.  Up to 2M Gaussians ~n / 1,024 buckets (up to 4,096) of <= 2,048
// items sorted by 256-thread workgroups (config 2 one frame at a time +7.7 %, config 5 +9.7 %).
// Above, that kind's scatter measured slower than the LSD passes at 5M (config 3 orbit: 181
// against 141 us, profiles/r06d_kt_c3_orbit_bucket_it56.txt); there 512 big buckets of ~n / 512
// items (gsr_internal.h launch_bucket_sort_big), each sorted by one 1,024-thread workgroup in
// LDS: 124 us, config 3 orbit +2.1 % in flight, +1.7 % one frame at a time
// (profiles/r06k_big_buckets_c3_orbit.txt).  Knob 28: 1 (default) both kinds by size; 2 the
// test hook (64-item capacity, either kind); 3 the small-bucket kind at any size (A/B).
constexpr int64_t kBucketSortMaxN = (int64_t)2048 * 1024;
bool bkt_applies(const gsr_context* c, int64_t n) { return n > 0 && c->set.bucket_sort != 0; }
bool bkt_big(const gsr_context* c, int64_t n) { return c->set.bucket_sort != 3 && n > kBucketSortMaxN; }
int bkt_count(const gsr_context* c, int64_t n) { return bkt_big(c, n) ? gsr::kBigBuckets : bkt_count(n); }

// Row items per column-pass chunk (GSR_TUNE_COL_CHUNK 0): 1,024 up to the same 2M
// Gaussians (config 2: column scatter 26.0 -> 21.6 us, chain -2 us), 2,048 above (config 3:
// the doubled chunk count costs the count and scan +10 us), profiles/r05_ab_col_chunk.txt.
int col_chunk_for(const gsr_context* c) {
    return c->set.col_chunk ? c->set.col_chunk : (c->n <= kBucketSortMaxN ? 1024 : 2048);
}

// ---- rank-order self-check, once per process and device (gsr_probes.hip
// k_rank_order_check).  The sort and binning kernels rank with returning LDS atomics
// only on a gfx950 device that returned every same-address lane in lane order.
std::mutex g_rank_mu;
std::unordered_map<int, RankCheck> g_rank;

}  // namespace

int gsr::rank_check_device(RankCheck* out) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_rank_mu);
    RankCheck& rc = g_rank[dev];
    if (rc.state < 0) {
        hipDeviceProp_t prop{};
        HIP_TRY(hipGetDeviceProperties(&prop, dev));
        if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
            rc.state = 0;
        } else {
            HIP_TRY(gsr::rank_order_check(&rc.ops, &rc.bad));
            rc.state = rc.ops > 0 && rc.bad == 0 ? 1 : 0;
        }
    }
    if (out) *out = rc;
    return GSR_OK;
}

int gsr::default_rank_atomic() {
    const char* e = std::getenv("GSR_RANK_ATOMIC");
    return e && e[0] == '0' ? 0 : 1;
}

int gsr::ensure_static(gsr_context* c) {
    if (c->set.rank_atomic < 0) c->set.rank_atomic = default_rank_atomic();
    if (c->hist) return GSR_OK;
    {
        RankCheck rk;
        if (int rc = rank_check_device(&rk)) return rc;
        c->rank_ok = rk.state == 1;
    }
    if (int rc = c->hist.alloc(256 * (size_t)gsr::kMaxSortGroups)) return rc;
    // LSD digit totals / bucket totals + bucket starts
    if (int rc = c->totals.alloc(2 * (size_t)gsr::kMaxBuckets + 2)) return rc;
    if (int rc = c->bkt_split.alloc(2 * (size_t)gsr::kMaxBuckets)) return rc;
    if (int rc = c->wg.alloc((size_t)gsr::kMaxSortGroups)) return rc;
    if (int rc = c->stats.alloc(2)) return rc;
    if (int rc = c->dstats.alloc(4 + 4 * (size_t)gsr::kMaxSortGroups)) return rc;
    if (int rc = c->nlive.alloc(1)) return rc;
    if (int rc = c->binmeta.alloc(256 + 128)) return rc;
    if (int rc = c->gate.alloc(1)) return rc;
    if (int rc = c->kcut.alloc(1)) return rc;
    if (int rc = c->kcut_frame.alloc(1)) return rc;
    if (int rc = c->nfar.alloc(1)) return rc;
    if (int rc = c->sat.alloc(257 * 257)) return rc;   // grids <= 256 x 256 tiles
    if (int rc = c->dstats_far.alloc(4 + 4 * (size_t)gsr::kMaxSortGroups)) return rc;
    HIP_TRY(hipMemset(c->kcut, 0xff, sizeof(uint32_t)));
    HIP_TRY(hipMemset(c->stats, 0, 2 * sizeof(Stats)));
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&c->hstats), sizeof(Stats), hipHostMallocMapped));
    std::memset(c->hstats, 0, sizeof(Stats));
    HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&c->hstats_dev), c->hstats, 0));
    HIP_TRY(hipEventCreateWithFlags(&c->done_ev, hipEventDisableTiming));
    return GSR_OK;
}

int gsr::ensure_n(gsr_context* c, int64_t n) {
    if (n <= c->n_cap) return GSR_OK;
    const int64_t cap = std::max<int64_t>(n, 1024);
    HIP_TRY(hipDeviceSynchronize());
    if (int rc = c->rec.alloc(4 * (size_t)cap)) return rc;
    if (int rc = c->items[0].alloc((size_t)cap)) return rc;
    if (int rc = c->items[1].alloc((size_t)cap)) return rc;
    if (int rc = c->rect.alloc((size_t)cap)) return rc;
    if (int rc = c->srect.alloc((size_t)cap)) return rc;
    if (int rc = c->spans.alloc((size_t)cap)) return rc;
    // the bucket sort's 16-B records (allocated with the items, so gsr_reserve covers them
    // and a captured frame never allocates)
    if (int rc = c->bkt_rec.alloc((size_t)cap)) return rc;
    c->n_cap = cap;
    if (c->p_cap < 4 * cap) {
        const int64_t pc = std::min<int64_t>(std::max<int64_t>(4 * cap, 1 << 20), 0xffffffffLL);
        if (int rc = c->pairs[0].alloc((size_t)pc)) return rc;
        if (int rc = c->pairs[1].alloc((size_t)pc)) return rc;
        c->p_cap = pc;
    }
    return GSR_OK;
}

int gsr::ensure_pairs(gsr_context* c, int64_t p) {
    if (p <= c->p_cap) return GSR_OK;
    const int64_t pc = std::min<int64_t>(p, 0xffffffffLL);
    HIP_TRY(hipDeviceSynchronize());
    if (int rc = c->pairs[0].alloc((size_t)pc)) return rc;
    if (int rc = c->pairs[1].alloc((size_t)pc)) return rc;
    c->p_cap = pc;
    return GSR_OK;
}

namespace {

// Depth split buffers for the current tile grid (4 blocks per tile).
int ensure_split(gsr_context* c) {
    const int64_t blocks = 4 * (int64_t)c->ntiles;
    if (blocks <= c->split_cap) return GSR_OK;
    HIP_TRY(hipDeviceSynchronize());
    if (int rc = c->tbuf.alloc(64 * (size_t)blocks)) return rc;
    if (int rc = c->bflag.alloc((size_t)blocks)) return rc;
    c->split_cap = blocks;
    return GSR_OK;
}

hipEvent_t get_event(gsr_context* c) {
    if (!c->ev_pool.empty()) {
        hipEvent_t e = c->ev_pool.back();
        c->ev_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

// Record the boundary event that opens stage `stage` (stage == GSR_NUM_STAGES closes the frame).
void mark(gsr_context* c, int stage) {
    if (!c->timing || !c->timing_now) return;
    const bool want = (c->timing == 2) || stage == GSR_STAGE_BLEND || stage == GSR_STAGE_RESUME ||
                      stage == GSR_NUM_STAGES;
    if (!want) return;
    hipEvent_t e = get_event(c);
    if (!e) return;
    c->cur.ev[stage] = e;
    (void)hipEventRecord(e, c->stream);
}

// What ends a frame, after its last blend kernel: the closing stage mark, the frame's timing
// events, and the completion event.
int frame_done(gsr_context* c) {
    mark(c, GSR_NUM_STAGES);
    if (c->timing && c->timing_now) c->ev_frames.push_back(c->cur);
    c->cur = FrameEvents{};
    // At most one completion event in flight: while the last one is unread, later
    // frames skip the record (~3 us each). The overflow stats are sticky, so reading
    // them when that older frame completes still sees every overflow so far, and
    // gsr_sync drains the stream before it reads them.
    if (!c->pending && c->set.completion_events) {
        HIP_TRY(hipEventRecord(c->done_ev, c->stream));
        c->pending = true;
    }
    return GSR_OK;
}

// The frame's tile grid fits the binning path (row + column binning, packed rects) and the
// knob asks for it.
bool binning_grid(const gsr_context* c) { return c->set.tile_binning && c->fr.tiles_x <= 256 && c->fr.tiles_y <= 256; }

// The size rule of the buffers that hold one element (or a fixed few) per Gaussian and grow on
// their own: never fewer than 1,024.
size_t per_gaussian(int64_t n) { return (size_t)std::max<int64_t>(n, 1024); }

// The split point and the controller's epoch as phase B publishes them (Stats::split_pm).
uint32_t split_tag(const gsr_context* c) { return (uint32_t)c->ctl.split_pm | ((c->ctl.split_epoch & 0xffffu) << 16); }

// Depth split point after a frame that needed phase B: up by half, floor at 5/4 of the
// old point, no speculation.
void split_grow(gsr_context* c) {
    c->ctl.split_floor = std::min(1000, c->ctl.split_pm * 5 / 4 + 1);
    c->ctl.split_pm = std::min(1000, c->ctl.split_pm * 3 / 2 + 1);
    c->ctl.split_clean = 0;
    c->ctl.split_spec = false;
}

void hv_clear_spec(gsr_context* c) {
    reinterpret_cast<volatile Stats*>(c->hstats)->spec_miss = 0;
}

// Read the sticky stats of finished work; grow the pair buffer after an overflow.
// An overflow (pairs over capacity, a depth sort short of passes, or a speculative
// depth-split frame that needed phase B) is reported once here and remembered in
// overflow_seen until gsr_sync, so a blocking sync also reports what a non-blocking
// check inside a render call already consumed.  The depth split's controller runs here
// too (the counts phase B published for the finished frames).
int check_overflow(gsr_context* c, bool blocking) {
    if (!c->pending) {
        // with completion events off (stream capture) no event marks finished work: a
        // blocking check (gsr_sync) drains the device and reads the sticky words anyway,
        // so an overflow or a speculative miss is still reported there
        if (!blocking || c->set.completion_events || !c->hstats) return GSR_OK;
        HIP_TRY(hipDeviceSynchronize());
    } else if (blocking) {
        HIP_TRY(hipEventSynchronize(c->done_ev));
    } else if (hipEventQuery(c->done_ev) != hipSuccess) {
        return GSR_OK;
    }
    c->pending = false;
    const volatile Stats* hv = c->hstats;
    Stats s{};
    s.pairs_total = hv->pairs_total;
    s.pairs_eff = hv->pairs_eff;
    s.overflow = hv->overflow;
    s.depth_passes = hv->depth_passes;
    if (!s.overflow && hv->spec_miss) {
        // a speculative frame (no phase B queued) left a block unsaturated: drain, then
        // report it like an overflow (the caller re-renders) and stop speculating
        HIP_TRY(hipDeviceSynchronize());
        hv_clear_spec(c);
        split_grow(c);
        c->overflow_seen = true;
        return set_err(GSR_E_OVERFLOW, "depth split: a frame rendered without phase B left blocks unsaturated; "
                                       "re-render");
    }
    if (!s.overflow && c->ctl.split_seen) {
        // depth split point: up by half when phase A left blocks unsaturated (phase B
        // ran), down by an eighth after 8 checked frames in a row that needed no phase B,
        // never below 5/4 of the last point that needed it; when it cannot shrink any
        // further, the next frames speculate (no phase B queued)
        c->ctl.split_seen = false;
        const int64_t u = hv->split_unsat;
        if (hv->split_pm != split_tag(c)) {
            // the newest phase B ran at an earlier split point (frames in flight): no
            // evidence about the current one yet
        } else if (u == 0) {
            c->ctl.split_retry = kSplitRetry;   // a saturating view: the next turn-off retries soon
            if (++c->ctl.split_clean >= 8) {
                c->ctl.split_clean = 0;
                const int next = std::max(std::max(kSplitMinPm, c->ctl.split_floor), c->ctl.split_pm * 7 / 8);
                if (next >= c->ctl.split_pm) c->ctl.split_spec = true;
                c->ctl.split_pm = next;
            }
        } else {
            const int pm_old = c->ctl.split_pm;
            split_grow(c);   // phase A left blocks unsaturated
            // at or above the starting point, 2 % of the blocks or more left unsaturated
            // means tiles that see past the scene, which no split point saturates (phase B
            // would run on every frame, at a cost above the unsplit frame's): off at once
            // rather than in four growth steps (automatic mode; a forced split keeps growing)
            if (c->set.depth_split == 2 && pm_old >= 250 && u * 50 >= 4 * (int64_t)c->ntiles) c->ctl.split_pm = 1000;
            if (c->ctl.split_pm >= 1000) {
                // the split turned itself off: the next frames list the whole order's pairs.
                // Size the pair buffer for them now (the split frames' pairs scaled to the
                // whole order) rather than overflow and re-render a chunk
                const int64_t want = (int64_t)(s.pairs_total * 1000 / (unsigned)pm_old) * 5 / 4 + 4096;
                if (int rc = ensure_pairs(c, want)) return rc;
            }
        }
    }
    if (!s.overflow) {
        // lower the pass budget once 4 checked frames in a row needed fewer passes
        if (s.depth_passes >= 1 && (int)s.depth_passes < c->depth_budget) {
            c->depth_budget_seen = std::max(c->depth_budget_seen, (int)s.depth_passes);
            if (++c->depth_budget_streak >= 4) {
                c->depth_budget = c->depth_budget_seen;
                c->depth_budget_streak = 0;
                c->depth_budget_seen = 0;
            }
        } else {
            c->depth_budget_streak = 0;
            c->depth_budget_seen = 0;
        }
        return GSR_OK;
    }
    // frames queued after the event may still be running: drain them, then read the
    // sticky stats again, so that a pair overflow of one of them (bit 0) is seen and
    // the grown capacity covers its total too (ensure_pairs syncs again; cheap)
    HIP_TRY(hipDeviceSynchronize());
    s.overflow |= hv->overflow;
    if (hv->pairs_total > s.pairs_total) s.pairs_total = hv->pairs_total;
    c->overflow_seen = true;
    // a speculative miss in the same frames: stop speculating before the words are
    // cleared, or the re-render of this camera speculates (and misses) again
    if (hv->spec_miss) split_grow(c);
    if (s.overflow & 2u) {   // back to four launched passes
        c->depth_budget = 4;
        c->depth_budget_streak = 0;
        c->depth_budget_seen = 0;
    }
    if (s.overflow & 1u) {
        const int64_t want = (int64_t)(s.pairs_total + s.pairs_total / 4 + 4096);
        if (int rc = ensure_pairs(c, want)) return rc;
    }
    HIP_TRY(hipMemset(c->stats + 1, 0, sizeof(Stats)));
    std::memset(c->hstats, 0, sizeof(Stats));
    if (s.overflow & 1u)
        return set_err(GSR_E_OVERFLOW, "pair buffer overflowed (%llu pairs); grown to %lld; re-render",
                       (unsigned long long)s.pairs_total, (long long)c->p_cap);
    return set_err(GSR_E_OVERFLOW, "depth sort needed %u passes, %d were launched; re-render",
                   (unsigned)s.depth_passes, c->passes_launched);
}

int fill_frame(Frame& f, const gsr_camera* cam, int W, int H, int nx, int ny, int ws, int hs, float k) {
    if (!cam) return set_err(GSR_E_ARG, "null camera");
    if (W <= 0 || H <= 0 || W > 32768 || H > 32768)
        return set_err(GSR_E_ARG, "image size %dx%d out of range [1, 32768]", W, H);
    if (nx <= 0 || ny <= 0 || ws <= 0 || hs <= 0)
        return set_err(GSR_E_ARG, "bad tiling nx=%d ny=%d ws=%d hs=%d", nx, ny, ws, hs);
    std::memcpy(f.V, cam->V_matrix, sizeof f.V);
    std::memcpy(f.P, cam->P_matrix, sizeof f.P);
    std::memcpy(f.Rc, cam->r_cam, sizeof f.Rc);
    std::memcpy(f.RcT, cam->r_cam_T, sizeof f.RcT);
    std::memcpy(f.campos, cam->position, sizeof f.campos);
    f.znear = cam->nearClip;
    gsr_camera_intrinsics(cam, &f.fx, &f.fy);
    f.k = k;
    f.W = W;
    f.H = H;
    f.cover_w = (int)std::min<int64_t>((int64_t)nx * ws, W);
    f.cover_h = (int)std::min<int64_t>((int64_t)ny * hs, H);
    f.tiles_x = (W + GSR_TILE_PX - 1) / GSR_TILE_PX;
    f.tiles_y = (H + GSR_TILE_PX - 1) / GSR_TILE_PX;
    return GSR_OK;
}

// The scene arguments every frame entry point refuses.
int check_scene_args(const void* scene, int layout, int64_t n) {
    if (n < 0 || n > INT32_MAX) return set_err(GSR_E_ARG, "Gaussian count %lld out of range", (long long)n);
    if (n > 0 && !scene) return set_err(GSR_E_ARG, "null scene");
    if (layout != GSR_LAYOUT_SCENE_BLOCK && layout != GSR_LAYOUT_AOS && layout != GSR_LAYOUT_SCENE_BLOCK_4D &&
        layout != GSR_LAYOUT_SCENE_BLOCK_SH3)
        return set_err(GSR_E_ARG, "unknown scene layout %d", layout);
    return GSR_OK;
}

int ceil_log2(int64_t v) {
    int k = 0;
    while ((int64_t(1) << k) < v) k++;
    return k;
}

}  // namespace

// ------------------------------------------------------------------ context lifetime

extern "C" gsr_context* gsr_create(void) {
    gsr_context* c = new gsr_context();
    const char* e = std::getenv("GSR_BLEND_EXP");
    if (e && e[0] == '0') c->set.blend_exp = 0;   // the exact blend (bit-identical to the oracle)
    if (e && e[0] == '1') c->set.blend_exp = 1;
    return c;
}

extern "C" void gsr_destroy(gsr_context* c) {
    if (!c) return;
    (void)hipDeviceSynchronize();
    for (auto* l : c->lanes) gsr_destroy(l);
    for (auto s : c->lane_streams) (void)hipStreamDestroy(s);
    for (auto e : c->join_evs) (void)hipEventDestroy(e);
    for (auto e : c->alias_evs) (void)hipEventDestroy(e);
    if (c->fork_ev) (void)hipEventDestroy(c->fork_ev);
    if (c->alt_ev) (void)hipEventDestroy(c->alt_ev);
    if (c->pre_ev) (void)hipEventDestroy(c->pre_ev);
    if (c->hstats) (void)hipHostFree(c->hstats);
    if (c->done_ev) (void)hipEventDestroy(c->done_ev);
    for (auto e : c->ev_pool) (void)hipEventDestroy(e);
    for (auto& f : c->ev_frames)
        for (auto e : f.ev)
            if (e) (void)hipEventDestroy(e);
    delete c;   // the device buffers (DevBuf members) go here
}

extern "C" int gsr_reserve(gsr_context* c, int64_t n, int64_t pairs) {
    if (!c || n < 0 || pairs < 0) return set_err(GSR_E_ARG, "gsr_reserve: bad argument");
    std::lock_guard<std::mutex> lk(c->mu);
    if (int rc = ensure_static(c)) return rc;
    if (int rc = ensure_n(c, n)) return rc;
    return ensure_pairs(c, pairs);
}

// ------------------------------------------------------------------ frame pipeline

// The host side of a frame's preprocess: the frame constants, the workspace, the split
// controller and every per-frame decision (which sort follows, where the items go, packed
// rects, spans, partial records).  Launches nothing but the AoS transpose.
int gsr::preprocess_plan(gsr_context* c, const void* scene, int layout, int64_t n, const gsr_camera* cam,
                         int W, int H, int nx, int ny, int ws, int hs, float k, void* stream) {
    if (int rc = check_scene_args(scene, layout, n)) return rc;
    if (int rc = fill_frame(c->fr, cam, W, H, nx, ny, ws, hs, k)) return rc;
    if (int rc = ensure_static(c)) return rc;
    int rc_over = check_overflow(c, false);
    if (rc_over != GSR_OK && rc_over != GSR_E_OVERFLOW) return rc_over;
    if (int rc = ensure_n(c, n)) return rc;
    c->ntiles = c->fr.tiles_x * c->fr.tiles_y;
    if (int rc = c->ranges.reserve((size_t)c->ntiles)) return rc;
    c->stream = static_cast<hipStream_t>(stream);
    c->n = n;
    if (c->timing) {
        c->cur = FrameEvents{};
        c->cur.mode = c->timing;
        c->timing_now = (c->timing_count++ % c->timing_stride) == 0;
    }
    mark(c, GSR_STAGE_PREPROCESS);
    const float* arrays = nullptr;
    int64_t stride = scene_stride(n);
    if (layout == GSR_LAYOUT_AOS) {
        if (int rc = c->soa_tmp.reserve((size_t)GSR_SCENE_NARRAYS * (size_t)stride)) return rc;
        HIP_TRY(gsr::launch_aos_to_soa(static_cast<const gsr_gaussian*>(scene), n, c->soa_tmp, stride, c->stream));
        arrays = c->soa_tmp;
    } else {
        arrays = scene_arrays(scene);
    }
    // depth split: the controller turned it off (split point 1000) because phase A kept
    // leaving blocks unsaturated; a camera that moved elsewhere can bring back views whose
    // tiles all saturate, so after split_retry frames, once the camera differs from the
    // one it was turned off on (a fixed camera, or a 4D scene's fixed camera over time,
    // never retries) and has stopped there (the same camera two frames running: a camera
    // that keeps moving, e.g. an orbit, never retries — its threshold would always come
    // from another view, and the controller's evidence lags the frames queued ahead of
    // it), it is tried again from the starting point; each retry doubles the next wait,
    // up to kSplitRetryMax, until a retry finds a view whose tiles all saturate
    const bool still = std::memcmp(c->ctl.prev_view, c->fr.V, sizeof c->fr.V) == 0 &&
                       std::memcmp(c->ctl.prev_view + 16, c->fr.P, sizeof c->fr.P) == 0;
    std::memcpy(c->ctl.prev_view, c->fr.V, sizeof c->fr.V);
    std::memcpy(c->ctl.prev_view + 16, c->fr.P, sizeof c->fr.P);
    if (c->ctl.split_pm >= 1000 && split_wanted(c, n)) {
        if (c->ctl.split_off_frames == 0) {
            std::memcpy(c->ctl.split_off_view, c->fr.V, sizeof c->fr.V);
            std::memcpy(c->ctl.split_off_view + 16, c->fr.P, sizeof c->fr.P);
        }
        if (c->ctl.split_retry == 0) c->ctl.split_retry = kSplitRetry;
        c->ctl.split_off_frames = std::min(c->ctl.split_off_frames + 1, 1 << 30);
        const bool moved = std::memcmp(c->ctl.split_off_view, c->fr.V, sizeof c->fr.V) != 0 ||
                           std::memcmp(c->ctl.split_off_view + 16, c->fr.P, sizeof c->fr.P) != 0;
        if (c->ctl.split_off_frames >= c->ctl.split_retry && moved && still) {
            c->ctl.split_retry = std::min(2 * c->ctl.split_retry, kSplitRetryMax);
            c->ctl.split_off_frames = 0;
            split_restart(c, 250);
        }
    } else {
        c->ctl.split_off_frames = 0;
    }
    // depth split with a depth threshold (a threshold exists from an earlier split
    // frame): the items go to src_items, which both sorts' pass 0 read
    c->split_key = split_enabled(c, n) && c->ctl.split_key_ready && binning_grid(c);
    // live partition (global depth sort on the binning path): the items go to
    // items[1] and the partition writes the visible-first order into items[0]
    // bucket depth sort (splitters exist for this scene size): the items go to items[1], the
    // sort writes the order into items[0]; it keeps culled items apart itself, so it
    // replaces the live partition
    // the splitters are this scene's and did not just fail: a frame whose global path sorted
    // more than n / 8 item-passes (a camera cut, a zoom: most of the scene in a few buckets
    // over capacity, with wide key spans) makes the next one reseed them from the LSD passes
    // (a camera jump could put most of a 2M scene into one bucket, sorted by one
    // workgroup, a frame of tens of ms).  Buckets of tied keys cost the global path nothing
    // (no passes) and do not count: reseeding could not split them.  bkt_over_work is
    // host-mapped and lags by the frames in flight; the test hook 2 (capacity 64) keeps them.
    {
        const unsigned int work = c->hstats ? ((const volatile Stats*)c->hstats)->bkt_over_work : 0u;
        const bool spike = c->set.bucket_sort != 2 && (int64_t)(work - c->bkt_work_seen) > n / 8;
        c->bkt_work_seen = work;
        if (c->bkt_B && (spike || c->bkt_scene != scene)) c->bkt_B = 0;
    }
    c->bds_frame = bkt_applies(c, n) && !c->split_key && c->set.bucket_sort && c->bkt_B == bkt_count(c, n) &&
                   binning_grid(c);
    c->compact_frame = n > 0 && !c->split_key && !c->bds_frame &&
                       (c->set.depth_compact == 1 || (c->set.depth_compact == 2 && layout == GSR_LAYOUT_SCENE_BLOCK_4D)) &&
                       binning_grid(c);
    // the binning path takes the tile rects packed to 4 B (pack_rect), the pair path 8 B;
    // the sort follows the path chosen here (rect_packed)
    c->rect_packed = binning_grid(c);
    // tile row spans: the row pass gathers each source's 2-B code by index; up to 1.5M
    // Gaussians the codes (<= 3 MB) stay in an XCD's 4-MB L2 and the gather is cheap:
    // config 2 (1M) +0.8 % one frame at a time, +1.2 % in flight; config 5 (2M) -1 % in
    // flight, config 3 (5M) -3 / -6 % (profiles/r02_ab_tile_spans.txt)
    c->spans_frame = c->rect_packed && (c->set.tile_spans == 1 || (c->set.tile_spans == 2 && n <= kLargeScene));
    // key mode: records only for the Gaussians nearer than the threshold (the far ones
    // are written by a second pass if phase B or a one-phase sort needs them)
    // (speculative frames only: a frame that queues phase B needs every record there)
    c->records_partial = c->split_key && c->ctl.split_spec && !c->spans_frame;
    c->pre_arrays = arrays;
    c->pre_scene = scene;
    c->pre_stride = stride;
    c->pre_layout = layout;
    if (c->split_key) {   // key mode: the preprocess order of n items
        if (int rc = c->src_items.reserve(per_gaussian(n))) return rc;
    }
    c->pre_out = c->split_key ? c->src_items : c->items[c->compact_frame || c->bds_frame ? 1 : 0];
    return rc_over;
}

// The planned frame's preprocess is queued (by preprocess_launch or a shared launch).
void gsr::preprocess_queued(gsr_context* c) {
    c->have_pre = true;
    c->have_sort = false;
}

int gsr::preprocess_launch(gsr_context* c, hipStream_t s) {
    const gsr::RecSplit rsp{c->records_partial ? 1 : 0, c->kcut, c->kcut_frame, nullptr};
    HIP_TRY(gsr::launch_preprocess(c->pre_arrays, c->pre_stride, c->n, c->fr, c->rec, c->pre_out,
                                   c->rect,
                                   c->rect_packed, c->pre_layout == GSR_LAYOUT_SCENE_BLOCK_4D,
                                   c->pre_layout == GSR_LAYOUT_SCENE_BLOCK_SH3, c->time, s,
                                   c->spans_frame ? c->spans : nullptr, &rsp));
    preprocess_queued(c);
    return GSR_OK;
}

int gsr::preprocess_locked(gsr_context* c, const void* scene, int layout, int64_t n, const gsr_camera* cam,
                           int W, int H, int nx, int ny, int ws, int hs, float k, void* stream) {
    const int rc = preprocess_plan(c, scene, layout, n, cam, W, H, nx, ny, ws, hs, k, stream);
    if (rc != GSR_OK && rc != GSR_E_OVERFLOW) return rc;
    if (int r2 = preprocess_launch(c, c->stream)) return r2;
    return rc;
}

static void* pair_keys(gsr_context* c, int b) { return c->pairs[b]; }

// Column-pass chunk counts for the current capacity and grid.
static int ensure_cbins(gsr_context* c) {
    return c->cbins.reserve(256 * (size_t)gsr::bin_col_chunks_max((uint32_t)c->p_cap, c->fr.tiles_y));
}

// Ranks from returning LDS atomics: asked for (GSR_TUNE_RANK_ATOMIC) and verified on the device.
static bool rank_atomic_on(const gsr_context* c) { return c->set.rank_atomic > 0 && c->rank_ok; }

// Rect payload buffer b (0 or 1) of the binning's depth sort: the two u32 halves of srect.
static uint32_t* pay_buf(gsr_context* c, int b) {
    return reinterpret_cast<uint32_t*>(c->srect.get()) + (b ? c->n_cap : 0);
}

// Global stable depth sort of the preprocess items (key << 32 | index), 4 x 8-bit
// passes with the device-side pass plan; with rects (binning) the passes carry them and
// leaves them in depth order (pay_buf(c, passes run & 1)).  Result in items[passes run & 1].
static int depth_sort_locked(gsr_context* c, bool with_rects, bool plain = false) {
    const uint32_t n = (uint32_t)c->n;
    c->bkt_rows_fused = false;
    // bucket depth sort: the first sort of a frame whose preprocess prepared for it (a
    // repeated sort of the frame takes the LSD passes over the sorted items[0])
    if (with_rects && !c->split_key && c->bds_frame && !c->have_sort && c->pre_out != c->items[0]) {
        const int B = c->bkt_B;
        if (bkt_big(c, c->n)) {
            // 512 buckets of ~n / 512 items, four 2,048-item tiles per scatter workgroup; the row
            // pass counts for itself (its 2,048-source chunks are cheaper than bucket chunks)
            const int G = std::min(groups_for(c->n, 4 * gsr::kMaxBucketCap), gsr::kBigBucketGroups);
            uint32_t* s_in = c->bkt_split + (size_t)c->bkt_par * gsr::kMaxBuckets;
            uint32_t* s_out = c->bkt_split + (size_t)(c->bkt_par ^ 1) * gsr::kMaxBuckets;
            HIP_TRY(gsr::launch_bucket_sort_big(c->pre_out, c->items[0], c->items[1], n, B, G, s_in, s_out, c->hist,
                                                c->totals, reinterpret_cast<const uint32_t*>(c->rect.get()), pay_buf(c, 0),
                                                pay_buf(c, 1), rank_atomic_on(c), c->set.bucket_sort == 2 ? 64u : 16384u,
                                                c->hstats_dev ? &c->hstats_dev->bkt_over : nullptr, c->stream,
                                                c->bkt_rec));
            c->bkt_rows_fused = false;
            c->bkt_par ^= 1;
            c->last_bds = true;
            c->last_compact = false;
            c->last_split_key = false;
            c->compact_frame = false;
            c->bds_frame = false;
            c->passes_launched = 4;
            return GSR_OK;
        }
        const int G = std::min(groups_for(c->n, gsr::kMaxBucketCap), gsr::kMaxBucketGroups);
        // a plain frame (one binning over the whole order): the local sorts also count the
        // row pass's items and pairs per bucket, which becomes the row pass's chunk
        const bool fuse = plain && c->set.fuse_rows && (int64_t)512 * B <= 256 * (int64_t)gsr::kMaxSortGroups;
        uint32_t* s_in = c->bkt_split + (size_t)c->bkt_par * gsr::kMaxBuckets;
        uint32_t* s_out = c->bkt_split + (size_t)(c->bkt_par ^ 1) * gsr::kMaxBuckets;
        HIP_TRY(gsr::launch_bucket_sort(c->pre_out, c->items[0], c->items[1], n, B, G, s_in, s_out, c->hist,
                                        c->totals, reinterpret_cast<const uint32_t*>(c->rect.get()), pay_buf(c, 0),
                                        pay_buf(c, 1), rank_atomic_on(c), c->set.bucket_sort == 2 ? 64u : gsr::kMaxBucketCap,
                                        c->hstats_dev ? &c->hstats_dev->bkt_over : nullptr, c->stream,
                                        fuse ? c->fr.tiles_y : 0, c->bkt_rec));
        c->bkt_rows_fused = fuse;
        c->bkt_par ^= 1;
        c->last_bds = true;
        c->last_compact = false;
        c->last_split_key = false;
        c->compact_frame = false;
        c->bds_frame = false;
        c->passes_launched = 4;   // no pass plan on this frame: the column scan's depth check is off
        return GSR_OK;
    }
    c->last_bds = false;
    // smaller tiles for the 1M-item depth sort: ~500 workgroups instead of ~250 (-2.6 %
    // frame time one at a time; in flight 8 and 16 measure within 1.5 % of each other,
    // either way round: profiles/r02_ab_depth_items.txt)
    // depth split, key mode: pass 0 reads the whole preprocess order (src_items) and keeps
    // the keys below the threshold; the passes sort only that near part (its count goes to
    // nlive; about 2 x the split point's items), the far part is sorted inside phase B
    const bool key = with_rects && c->split_key;
    const int64_t n_sorted =
        key ? std::min<int64_t>(c->n, std::max<int64_t>(2 * ((int64_t)c->n * c->ctl.split_pm / 1000), 65536)) : c->n;
    const int di = c->set.depth_items ? c->set.depth_items : (n_sorted < (int64_t(4) << 20) ? 8 : 16);
    int gd = groups_for(key ? c->n : n_sorted, 256 * di);   // pass 0 reads all n
    int gd_near = groups_for(n_sorted, 256 * di);
    if (c->set.depth_groups) {
        gd = std::min(gd, c->set.depth_groups);
        gd_near = std::min(gd_near, c->set.depth_groups);
    }
    const bool part = with_rects && c->compact_frame;
    // visible items first (index order) into items[0]; the passes sort only those
    if (part)
        HIP_TRY(gsr::launch_partition(c->pre_out, n, std::min(groups_for(c->n, 4096), gsr::kMaxSortGroups), c->hist,
                                      c->nlive, c->items[0], reinterpret_cast<const uint32_t*>(c->rect.get()),
                                      pay_buf(c, 0), pay_buf(c, 1), c->stream));
    // a repeated sort of a key-mode frame starts again from the preprocess order
    const bool resort_src = !key && !part && c->have_sort && c->last_split_key;
    if (resort_src)
        HIP_TRY(hipMemcpyAsync(c->items[0], c->src_items, (size_t)n * 8, hipMemcpyDeviceToDevice, c->stream));
    c->last_compact = part;
    c->last_split_key = key;
    if (key) c->split_key = false;
    // pass 0's rect payloads: from the partition (-1), read at the item's position when
    // the input is the preprocess order (1: item j has index j), else gathered (0)
    const int rect_mode = part ? -1 : (key || resort_src || !c->have_sort ? 1 : 0);
    // items[1] is the sort's scratch from here on; a repeated sort of this frame sorts
    // the whole partitioned items[0] (same order: visible and culled keys never tie)
    if (part) c->compact_frame = false;
    // Trailing passes the device plan skips still cost a launch each (upsweep, scan and
    // downsweep returning at once: ~12 us of the frame's dependent chain).  On the
    // binning path the host launches only as many passes as recent frames needed
    // (depth_budget, check_overflow); a frame that needs more is flagged by the
    // column scan and re-rendered with all four, like a pair-buffer overflow.
    const int launch = with_rects && c->set.depth_skip ? std::max(1, std::min(4, c->depth_budget)) : 4;
    c->passes_launched = launch;
    const gsr::SortFilter near{1, c->kcut, c->nlive, c->kcut_frame};
    for (int p = 0; p < launch; p++) {
        const bool f0 = key && p == 0;
        HIP_TRY(gsr::launch_radix_pass(f0 ? c->src_items : c->items[p & 1], c->items[(p + 1) & 1],
                                       (part || (key && p > 0)) ? c->nlive : nullptr, n, 32 + 8 * p, 8,
                                       key && p > 0 ? gd_near : gd, di,
                                       c->hist, c->totals, nullptr, c->stream, c->set.depth_skip ? c->dstats : nullptr,
                                       p, with_rects ? reinterpret_cast<const uint32_t*>(c->rect.get()) : nullptr, rect_mode,
                                       with_rects ? pay_buf(c, 0) : nullptr,
                                       with_rects ? pay_buf(c, 1) : nullptr, rank_atomic_on(c), nullptr, nullptr,
                                       f0 ? &near : nullptr));
    }
    // the bucket sort's first splitters: quantiles of this whole sorted order (the next
    // frame of this scene size is bucket-sorted)
    if (with_rects && !key && c->set.bucket_sort && bkt_applies(c, c->n) && c->bkt_B != bkt_count(c, c->n)) {
        const int B = bkt_count(c, c->n);
        HIP_TRY(gsr::launch_bkt_splitters(c->items[0], c->items[1], c->set.depth_skip ? c->dstats : nullptr, n,
                                          part ? c->nlive : nullptr, B,
                                          c->bkt_split + (size_t)c->bkt_par * gsr::kMaxBuckets, c->stream));
        c->bkt_B = B;
        c->bkt_scene = c->pre_scene;
    }
    return GSR_OK;
}

// Depth split, key mode, phase B: the far part [nlive, n) sorted on its own (its own
// pass plan), every kernel returning at once when phase A saturated every block.
static int far_sort_locked(gsr_context* c) {
    const uint32_t n = (uint32_t)c->n;
    const int di = c->set.depth_items ? c->set.depth_items : (c->n < (int64_t(4) << 20) ? 8 : 16);
    int gd = groups_for(c->n, 256 * di);
    if (c->set.depth_groups) gd = std::min(gd, c->set.depth_groups);
    // the pass budget follows the near sorts (phase A's column scan reports them, and
    // their key range can be far narrower); the far keys get at least three passes
    // (keys below 2^24, depths under 16.7), so a phase B is rarely short of passes
    const int launch = c->set.depth_skip ? std::max(3, std::min(4, c->depth_budget)) : 4;
    c->far_launched = launch;
    // the summed-area table of the tiles phase A left unsaturated; pass 0 reads the whole
    // preprocess order and keeps the items with keys at or above the frame's threshold
    // whose rect touches such a tile, writing them from position nlive (count in nfar);
    // the later passes sort [nlive, nlive + nfar)
    HIP_TRY(gsr::launch_split_sat(c->bflag, c->fr.tiles_x, c->fr.tiles_y, c->sat, c->gate, c->stream));
    const gsr::SortFilter far{2, c->kcut_frame, c->nfar, nullptr, c->sat, c->fr.tiles_x + 1, nullptr};
    const gsr::SortFilter rest{0, nullptr, nullptr, nullptr, nullptr, 0, c->nfar};
    for (int p = 0; p < launch; p++)
        HIP_TRY(gsr::launch_radix_pass(p == 0 ? c->src_items : c->items[p & 1], c->items[(p + 1) & 1], nullptr, n,
                                       32 + 8 * p, 8, gd, di, c->hist, c->totals, nullptr, c->stream,
                                       c->set.depth_skip ? c->dstats_far : nullptr, p,
                                       reinterpret_cast<const uint32_t*>(c->rect.get()), p == 0 ? 1 : 0, pay_buf(c, 0),
                                       pay_buf(c, 1), rank_atomic_on(c), c->nlive, c->gate, p == 0 ? &far : &rest));
    return GSR_OK;
}

// The far Gaussians' records, when the preprocess wrote only the near ones (key mode):
// gated = phase B (returns at once when phase A saturated every block), else always.
int gsr::far_records_locked(gsr_context* c, bool gated) {
    if (!c->records_partial) return GSR_OK;
    const gsr::RecSplit rsp{2, nullptr, c->kcut_frame, gated ? c->gate : nullptr};
    HIP_TRY(gsr::launch_preprocess(c->pre_arrays, c->pre_stride, c->n, c->fr, c->rec, c->items[0], c->rect,
                                   c->rect_packed, c->pre_layout == GSR_LAYOUT_SCENE_BLOCK_4D,
                                   c->pre_layout == GSR_LAYOUT_SCENE_BLOCK_SH3, c->time, c->stream, nullptr, &rsp));
    if (!gated) c->records_partial = false;
    return GSR_OK;
}

// Row pass, then column pass (gsr_kernels.hip "tile binning") over the depth-order
// positions [base, base + count): tile lists in pair_vals(c, 1), ranges.  gate_mode:
// 0 plain; 1 = depth split phase A (clears the gate); 2 = phase B (every kernel returns
// at once when the gate is 0).
// rs (nullable): the depth split's device-side ranges and threshold update; far: the
// positions were sorted by far_sort_locked (its pass plan and pass count apply).
static int bin_locked(gsr_context* c, uint32_t base, uint32_t count, int gate_mode, bool marks,
                      const gsr::RowSplit* rs = nullptr, bool far = false) {
    const uint32_t cap = (uint32_t)c->p_cap;
    if (int rc = ensure_cbins(c)) return rc;
    auto* row_pairs = reinterpret_cast<unsigned long long*>(c->binmeta.get());
    auto* row_items = reinterpret_cast<uint32_t*>(c->binmeta + 256);
    // key mode, phase A: about 2 x the split point's items (the count is on the device)
    const int64_t est = rs && rs->cut_mode == 1 ? std::min<int64_t>(count, std::max<int64_t>(2 * (int64_t)rs->na, 65536))
                                                : (int64_t)count;
    // Sources per row-pass chunk (rounded up to a multiple of 1,024, the chunks capped at
    // 4,096): 1,024, and 3,072 for a whole-order pass above 2M Gaussians (config 3 orbit, big
    // buckets: the row pass 72.8 -> 65.8 us, the count and scan pay per chunk and the scatter
    // takes 3,072 sources as well as ~1,200; 4,096: 68.7, profiles/r06o_kt_row_chunk_c3.txt).
    const int64_t row_chunk = !rs && est > kBucketSortMaxN ? 3072 : 1024;
    const int gb = std::min(groups_for(est, row_chunk), gsr::kMaxSortGroups / 2);
    // (a bucket-sorted frame has no pass plan: its order is in items[0], its rects in pay_buf 0)
    uint32_t* dst = c->set.depth_skip && !(c->last_bds && !far) ? (far ? c->dstats_far : c->dstats) : nullptr;
    // after a bucket-sorted plain frame the buckets are the row chunks and their counts exist
    const bool fused = c->bkt_rows_fused && gate_mode == 0 && base == 0 && !rs && !far && count == (uint32_t)c->n;
    c->bkt_rows_fused = false;
    const uint32_t* cstart = fused ? c->totals + c->bkt_B : nullptr;
    HIP_TRY(gsr::launch_bin_rows(c->items[0], c->items[1], dst, count, pay_buf(c, 0),
                                 pay_buf(c, 1), fused ? c->bkt_B : gb,
                                 c->hist, row_items, row_pairs, cap, c->fr.tiles_y, c->pairs[0], c->set.bin_row_items,
                                 c->stream, c->spans_frame ? c->spans : nullptr, rank_atomic_on(c), base,
                                 gate_mode ? c->gate : nullptr, gate_mode, rs && rs->cut_mode ? c->nlive : nullptr,
                                 rs, cstart));
    if (marks) mark(c, GSR_STAGE_TILE_SORT);
    // column-pass workgroups: ~one 2048-item chunk each (config 3: 2048-4096 groups 12 us
    // faster than 1024; config 2: 1024 best, profiles/r02_ab_col_groups.txt)
    const int gcol = c->set.bin_col_groups ? c->set.bin_col_groups
                                       : (int)std::min<int64_t>(4096, std::max<int64_t>(1024, c->n / 1024));
    HIP_TRY(gsr::launch_bin_cols(c->pairs[0], row_items, row_pairs, c->cbins, gcol, cap,
                                 c->fr.tiles_x, c->fr.tiles_y, pair_vals(c, 1), c->ranges, c->stats,
                                 c->hstats_dev, c->set.bin_col_items, c->stream,
                                 dst, far ? c->far_launched : c->passes_launched, rank_atomic_on(c),
                                 gate_mode == 2 ? c->gate : nullptr, c->fstatus, col_chunk_for(c)));
    c->pair_buf = 1;
    return GSR_OK;
}

// allow_split: the caller blends right after (gsr_render, gsr_render_path), so the
// depth split may apply (the stage API gsr_sort / gsr_blend keeps one phase).
int gsr::sort_locked(gsr_context* c, bool allow_split) {
    if (!c->have_pre) return set_err(GSR_E_ARG, "gsr_sort before gsr_preprocess");
    const uint32_t n = (uint32_t)c->n;
    const bool bin = c->rect_packed;   // the path gsr_preprocess chose (its rect format)
    c->last_binned = bin;
    c->split_state_hold = -1;
    // depth split for this frame (gsr_render / gsr_render_path on the binning path):
    // count mode sorts the whole order and phase A bins its nearest na positions; key
    // mode (a threshold from an earlier split frame exists) partitions by the threshold
    // and sorts only the near part, which phase A bins
    const uint32_t na = (uint32_t)std::max<int64_t>(1, ((int64_t)n * c->ctl.split_pm + 999) / 1000);
    const bool split = bin && allow_split && split_enabled(c, c->n) && na < n;
    if (c->split_key && !split) {   // preprocessed for key mode: sort every visible item instead
        c->split_key = false;
        c->compact_frame = true;
    }
    if ((c->compact_frame || c->bds_frame) && !bin) {   // knobs changed since gsr_preprocess
        HIP_TRY(hipMemcpyAsync(c->items[0], c->pre_out, (size_t)n * 8, hipMemcpyDeviceToDevice, c->stream));
        c->compact_frame = false;
        c->bds_frame = false;
    }
    const bool key = split && c->split_key;
    if (!key) {   // a frame preprocessed for key mode that is not split that way: all records
        if (int rc = far_records_locked(c, false)) return rc;
    }
    // ---- stable depth sort of (key << 32 | index), 4 x 8 bits; for the binning
    // path the passes carry the rects, depth-ordered at the end (pay_buf) ----
    mark(c, GSR_STAGE_DEPTH_SORT);
    if (int rc = depth_sort_locked(c, bin, bin && !split)) return rc;
    // result in items[passes run & 1] (device-side plan; emission picks it)
    if (bin) {
        // depth split: phase A bins the near part (blend_locked blends it, then sorts
        // and bins the rest where needed)
        c->split_frame = split;
        c->split_rebin = false;
        c->frame_key = key;
        // speculate only when the camera is the one the threshold came from (a moving camera
        // would leave blocks unsaturated and cost a re-render)
        const bool same_view = std::memcmp(c->ctl.split_view, c->fr.V, sizeof c->fr.V) == 0 &&
                               std::memcmp(c->ctl.split_view + 16, c->fr.P, sizeof c->fr.P) == 0;
        // (and only with completion events on: a captured graph would bake "no phase B"
        // into every replay)
        c->frame_spec = split && key && c->ctl.split_spec && same_view && c->set.completion_events;
        if (split) {
            std::memcpy(c->ctl.split_view, c->fr.V, sizeof c->fr.V);
            std::memcpy(c->ctl.split_view + 16, c->fr.P, sizeof c->fr.P);
        }
        mark(c, GSR_STAGE_EMIT);
        if (split) {
            if (int rc = ensure_split(c)) return rc;
            c->split_na = na;
            const gsr::RowSplit rs{key ? 1 : 0, na, nullptr};
            if (int rc = bin_locked(c, 0, key ? n : na, 1, true, &rs)) return rc;
        } else {
            if (int rc = bin_locked(c, 0, n, 0, true)) return rc;
        }
        mark(c, GSR_STAGE_RANGES);
        c->have_sort = true;
        return GSR_OK;
    }
    // ---- pair emission in depth order (srect staged in the free items buffer) ----
    mark(c, GSR_STAGE_EMIT);
    const int ge = groups_for(c->n, 1024);
    const bool key16 = c->ntiles <= 65536;
    HIP_TRY(gsr::launch_emit(c->items[0], c->items[1], c->set.depth_skip ? c->dstats : nullptr, n, c->rect, ge, c->wg,
                             c->stats, c->hstats_dev, (uint32_t)c->p_cap, c->fr.tiles_x, c->fr.tiles_y,
                             pair_keys(c, 0), key16, pair_vals(c, 0), c->ranges, c->stream, c->fstatus));
    // ---- stable key-value tile sort ----
    mark(c, GSR_STAGE_TILE_SORT);
    const int tbits = std::max(1, ceil_log2(c->ntiles));
    int gp = groups_for(c->p_cap, 256 * c->set.tile_items);
    if (c->set.tile_groups) gp = std::min(gp, c->set.tile_groups);
    int cur = 0;
    // digits split evenly over the passes (13 bits: 7 + 6, not 8 + 5): longer
    // digit runs per sorted tile of items, so the scattered stores coalesce better
    const int tpasses = (tbits + 7) / 8;
    const int tdig = c->set.tile_split_even ? (tbits + tpasses - 1) / tpasses : 8;
    for (int sh = 0; sh < tbits; sh += tdig) {
        const int bits = std::min(tdig, tbits - sh);
        const bool last = sh + tdig >= tbits;    // final pass: values only + tile ranges
        HIP_TRY(gsr::launch_kv_pass(pair_keys(c, cur), pair_vals(c, cur), last ? nullptr : pair_keys(c, cur ^ 1),
                                    pair_vals(c, cur ^ 1), key16, &c->stats[0].pairs_eff, sh, bits, gp,
                                    c->set.tile_items, c->hist, c->totals, last ? c->ranges : nullptr, c->stream));
        cur ^= 1;
    }
    c->pair_buf = cur;
    mark(c, GSR_STAGE_RANGES);
    c->have_sort = true;
    return GSR_OK;
}

int gsr::blend_locked(gsr_context* c, float* d_out) {
    if (!c->have_sort) return set_err(GSR_E_ARG, "gsr_blend before gsr_sort");
    if (!d_out) return set_err(GSR_E_ARG, "null output");
    mark(c, GSR_STAGE_BLEND);
    if (c->diagnostics) {
        // counters (16) and the per-pixel take map, or, for the timestamp schedule,
        // 2 stamps per wave
        const int64_t need = c->blend_variant == 3 ? 12 * (int64_t)c->ntiles + 64   // >= 2 x the padded grid
                                                   : 16 + (int64_t)c->fr.W * c->fr.H;
        if ((int64_t)c->consumed.capacity() < need) {
            if (int rc = c->consumed.alloc((size_t)need)) return rc;
        }
        HIP_TRY(hipMemsetAsync(c->consumed, 0, (size_t)need * sizeof(unsigned long long), c->stream));
    }
    if (c->split_frame) {
        // depth split: blend phase A (saving the blocks it leaves unsaturated), bin the
        // rest of the depth order, resume those blocks; phase B's kernels return at once
        // on the device when phase A saturated every block
        const uint32_t n = (uint32_t)c->n;
        const bool key = c->frame_key;
        if (key && c->blend_variant == 3)
            return set_err(GSR_E_ARG, "gsr_blend: blend knobs changed after a depth-split frame; render it again");
        const gsr::RowSplit ra{key ? 1 : 0, c->split_na, nullptr};
        if (c->split_rebin && c->blend_variant != 3) {
            if (int rc = bin_locked(c, 0, key ? n : c->split_na, 1, false, &ra)) return rc;
        }
        if (c->blend_variant != 3) {
            // phase A; its workgroup 0 also sets the next frame's threshold from the near
            // depth order (key mode: the near part; count mode: the whole order)
            const bool spec = c->frame_spec;
            const gsr::SplitCut cut{c->items[0], c->items[1], c->set.depth_skip && !c->last_bds ? c->dstats : nullptr,
                                    key ? c->nlive : nullptr, n, c->split_na, c->split_rebin ? nullptr : c->kcut};
            gsr::BlendSplit a{1, c->tbuf, c->bflag, c->gate, nullptr, spec ? c->hstats_dev : nullptr, cut, 0u,
                              spec ? c->fstatus : nullptr};
            HIP_TRY(gsr::launch_blend(pair_vals(c, c->pair_buf), c->ranges, c->rec, c->fr, d_out,
                                      c->diagnostics ? c->consumed : nullptr, false, c->set.blend_band_tiles, 0,
                                      c->stream, &a));
            c->ctl.split_key_ready = true;
            mark(c, GSR_STAGE_RESUME);
            if (!spec) {
                // phase B: (key mode) sort the far part, then bin the rest of the order
                const gsr::RowSplit rb{key ? 2 : 0, c->split_na, key ? c->nfar : nullptr};
                if (key && !c->split_rebin) {
                    if (int rc = far_sort_locked(c)) return rc;
                    if (int rc = far_records_locked(c, true)) return rc;
                }
                if (int rc = bin_locked(c, key ? 0 : c->split_na, key ? n : n - c->split_na, 2, false, &rb, key))
                    return rc;
                // (cut: only the near count and the split point, for the published tag)
                const gsr::SplitCut bcut{nullptr, nullptr, nullptr, key ? c->nlive : nullptr, n, c->split_na, nullptr};
                gsr::BlendSplit b{2, c->tbuf, c->bflag, c->gate, c->hstats_dev, nullptr, bcut, split_tag(c),
                                  nullptr};
                HIP_TRY(gsr::launch_blend(pair_vals(c, c->pair_buf), c->ranges, c->rec, c->fr, d_out,
                                          c->diagnostics ? c->consumed : nullptr, false, c->set.blend_band_tiles, 0,
                                          c->stream, &b));
                c->ctl.split_seen = true;
            }
            c->split_rebin = true;
        } else {
            // knobs changed since the sort: bin the whole depth order again, one phase
            if (int rc = bin_locked(c, 0, (uint32_t)c->n, 0, false)) return rc;
            c->split_frame = false;
            HIP_TRY(gsr::launch_blend(pair_vals(c, c->pair_buf), c->ranges, c->rec, c->fr, d_out,
                                      c->diagnostics ? c->consumed : nullptr, c->blend_variant == 3,
                                      c->set.blend_band_tiles, c->set.blend_exp, c->stream));
        }
    } else {
        HIP_TRY(gsr::launch_blend(pair_vals(c, c->pair_buf), c->ranges, c->rec, c->fr, d_out,
                                  c->diagnostics ? c->consumed : nullptr, c->blend_variant == 3,
                                  c->set.blend_band_tiles, c->set.blend_exp, c->stream));
    }
    return frame_done(c);
}

// ------------------------------------------------------------------ stage API, gsr_render

extern "C" int gsr_preprocess(gsr_context* c, const void* scene, int layout, int64_t n, const gsr_camera* cam,
                              int W, int H, int nx, int ny, int ws, int hs, float k, void* stream) {
    if (!c) return set_err(GSR_E_ARG, "null context");
    std::lock_guard<std::mutex> lk(c->mu);
    return preprocess_locked(c, scene, layout, n, cam, W, H, nx, ny, ws, hs, k, stream);
}

extern "C" int gsr_sort(gsr_context* c, void* stream) {
    if (!c) return set_err(GSR_E_ARG, "null context");
    std::lock_guard<std::mutex> lk(c->mu);
    c->stream = static_cast<hipStream_t>(stream);
    return sort_locked(c, false);
}

extern "C" int gsr_blend(gsr_context* c, float* d_out, void* stream) {
    if (!c) return set_err(GSR_E_ARG, "null context");
    std::lock_guard<std::mutex> lk(c->mu);
    c->stream = static_cast<hipStream_t>(stream);
    return blend_locked(c, d_out);
}

extern "C" int gsr_render(gsr_context* c, const void* scene, int layout, int64_t n, const gsr_camera* cam, int W,
                          int H, int nx, int ny, int ws, int hs, float k, float* d_out, void* stream) {
    if (!c) return set_err(GSR_E_ARG, "null context");
    std::lock_guard<std::mutex> lk(c->mu);
    int rc = preprocess_locked(c, scene, layout, n, cam, W, H, nx, ny, ws, hs, k, stream);
    if (rc != GSR_OK && rc != GSR_E_OVERFLOW) return rc;
    if (int r2 = sort_locked(c, true)) return r2;
    if (int r3 = blend_locked(c, d_out)) return r3;
    return rc;
}

// ------------------------------------------------------------------ auxiliary render targets

namespace {

// The sorted frame's blend with auxiliary targets: blend_locked's one-phase frame with
// k_blend_aux in place of k_blend_w, and no diagnostics.
int blend_aux_locked(gsr_context* c, float* d_out, const gsr_aux_targets& aux) {
    const bool with_z = aux.d_depth && c->n > 0;
    if (with_z) {   // -Z per Gaussian
        if (int rc = c->aux_z.reserve(per_gaussian(c->n))) return rc;
    }
    if (aux.nfeat > 4 && c->n > 0) {   // more than four features: their interleaved copy, 2 float4 per Gaussian
        if (int rc = c->aux_pack.reserve(2 * per_gaussian(c->n))) return rc;
    }
    mark(c, GSR_STAGE_BLEND);   // the stage holds the -Z and feature-pack kernels too
    if (with_z)
        HIP_TRY(gsr::launch_aux_depth(c->pre_arrays, c->pre_stride, c->n, c->fr,
                                      c->pre_layout == GSR_LAYOUT_SCENE_BLOCK_4D, c->time, c->aux_z, c->stream));
    HIP_TRY(gsr::launch_blend_aux(pair_vals(c, c->pair_buf), c->ranges, c->rec, c->fr, d_out, aux.d_alpha,
                                  aux.d_depth, c->aux_z, aux.d_features, c->n, aux.nfeat, aux.d_feat_out, c->aux_pack,
                                  c->set.blend_band_tiles, c->stream));
    return frame_done(c);
}

// The sorted frame's contribution statistics (gsr_render_contrib): k_blend_contrib in place
// of k_blend_w, under GSR_STAGE_BLEND, no diagnostics.  The kernel reads the frame's
// overflow word (stats[0], written by the binning / emission kernels queued before it).
int blend_contrib_locked(gsr_context* c, const gsr_contrib_targets& out) {
    mark(c, GSR_STAGE_BLEND);
    HIP_TRY(gsr::launch_blend_contrib(pair_vals(c, c->pair_buf), c->ranges, c->rec, c->fr, out.d_count,
                                      reinterpret_cast<unsigned long long*>(out.d_weight), out.d_max, out.d_id,
                                      &c->stats[0].overflow, c->set.blend_band_tiles, c->stream));
    return frame_done(c);
}

// The sorted frame's backward pass (gsr_render_backward): k_blend_backward in place of
// k_blend_w, under GSR_STAGE_BLEND, no diagnostics; the overflow word as above.
int blend_backward_locked(gsr_context* c, const gsr_backward_targets& bw) {
    mark(c, GSR_STAGE_BLEND);
    HIP_TRY(gsr::launch_blend_backward(pair_vals(c, c->pair_buf), c->ranges, c->rec, c->fr, bw.d_grad_image,
                                       bw.d_grad_alpha, bw.d_color, bw.d_opacity, bw.d_conic, bw.d_center, c->n,
                                       &c->stats[0].overflow, c->set.blend_band_tiles, c->stream));
    return frame_done(c);
}

// The frame policy of gsr_render_aux and gsr_render_contrib, around the frame's own blend.
// One phase, exact blend, and the depth split's controller untouched: the preprocess
// and the sort run with the split off (no threshold partition, no partial records, no
// retry bookkeeping), and what the preprocess's overflow check learned from earlier
// split frames is put back for the next non-aux frame's check to learn again (their
// evidence is sticky) — unless that check reported an incomplete frame, whose
// consequences (no more speculation) stand.
template <typename Blend>
int aux_frame_locked(gsr_context* c, const void* scene, int layout, int64_t n, const gsr_camera* cam, int W, int H,
                     int nx, int ny, int ws, int hs, float k, void* stream, Blend&& blend) {
    SplitCtl ctl = c->ctl;
    const int state = split_state(c);
    const int depth_split = c->set.depth_split;
    c->set.depth_split = 0;
    int rc = preprocess_locked(c, scene, layout, n, cam, W, H, nx, ny, ws, hs, k, stream);
    int r2 = GSR_OK;
    if (rc == GSR_OK || rc == GSR_E_OVERFLOW) {
        r2 = sort_locked(c, false);
        if (r2 == GSR_OK) r2 = blend();
        c->split_state_hold = state;
    }
    c->set.depth_split = depth_split;
    if (rc == GSR_E_OVERFLOW) {
        // the view bookkeeping only
        ctl.split_pm = c->ctl.split_pm;
        ctl.split_floor = c->ctl.split_floor;
        ctl.split_clean = c->ctl.split_clean;
        ctl.split_spec = c->ctl.split_spec;
        ctl.split_seen = c->ctl.split_seen;
    }
    c->ctl = ctl;
    if (rc != GSR_OK && rc != GSR_E_OVERFLOW) return rc;
    return r2 ? r2 : rc;
}

}  // namespace

extern "C" int gsr_render_aux(gsr_context* c, const void* scene, int layout, int64_t n, const gsr_camera* cam,
                              int W, int H, int nx, int ny, int ws, int hs, float k, float* d_out,
                              const gsr_aux_targets* aux, void* stream) {
    if (!c) return set_err(GSR_E_ARG, "null context");
    if (!aux) return set_err(GSR_E_ARG, "gsr_render_aux: null aux targets");
    if (aux->nfeat < 0 || aux->nfeat > GSR_AUX_MAX_FEATURES)
        return set_err(GSR_E_ARG, "gsr_render_aux: nfeat %d out of range [0, %d]", aux->nfeat, GSR_AUX_MAX_FEATURES);
    if (aux->nfeat > 0 && (!aux->d_features || !aux->d_feat_out))
        return set_err(GSR_E_ARG, "gsr_render_aux: nfeat %d needs d_features and d_feat_out", aux->nfeat);
    if (!d_out && !aux->d_alpha && !aux->d_depth && aux->nfeat == 0)
        return set_err(GSR_E_ARG, "gsr_render_aux: no output");
    std::lock_guard<std::mutex> lk(c->mu);
    return aux_frame_locked(c, scene, layout, n, cam, W, H, nx, ny, ws, hs, k, stream,
                            [&] { return blend_aux_locked(c, d_out, *aux); });
}

extern "C" int gsr_render_contrib(gsr_context* c, const void* scene, int layout, int64_t n, const gsr_camera* cam,
                                  int W, int H, int nx, int ny, int ws, int hs, float k,
                                  const gsr_contrib_targets* out, void* stream) {
    if (!c) return set_err(GSR_E_ARG, "null context");
    if (!out) return set_err(GSR_E_ARG, "gsr_render_contrib: null targets");
    if (!out->d_count && !out->d_weight && !out->d_max && !out->d_id)
        return set_err(GSR_E_ARG, "gsr_render_contrib: no output");
    std::lock_guard<std::mutex> lk(c->mu);
    return aux_frame_locked(c, scene, layout, n, cam, W, H, nx, ny, ws, hs, k, stream,
                            [&] { return blend_contrib_locked(c, *out); });
}

extern "C" int gsr_render_backward(gsr_context* c, const void* scene, int layout, int64_t n, const gsr_camera* cam,
                                   int W, int H, int nx, int ny, int ws, int hs, float k,
                                   const gsr_backward_targets* bw, void* stream) {
    if (!c) return set_err(GSR_E_ARG, "null context");
    if (!bw) return set_err(GSR_E_ARG, "gsr_render_backward: null targets");
    if (!bw->d_grad_image && !bw->d_grad_alpha)
        return set_err(GSR_E_ARG, "gsr_render_backward: no upstream gradient");
    if (!bw->d_color && !bw->d_opacity && !bw->d_conic && !bw->d_center)
        return set_err(GSR_E_ARG, "gsr_render_backward: no output");
    std::lock_guard<std::mutex> lk(c->mu);
    return aux_frame_locked(c, scene, layout, n, cam, W, H, nx, ny, ws, hs, k, stream,
                            [&] { return blend_backward_locked(c, *bw); });
}

// ------------------------------------------------------------------ projection backward

namespace {

// What gsr_project_backward and gsr_render_backward_scene refuse beyond a frame's arguments.
int check_scene_grads(const char* who, const gsr_scene_grads* out, int layout) {
    if (!out) return set_err(GSR_E_ARG, "%s: null outputs", who);
    if (!out->d_position && !out->d_opacity && !out->d_scale && !out->d_rot && !out->d_sh && !out->d_temporal)
        return set_err(GSR_E_ARG, "%s: no output", who);
    if (layout == GSR_LAYOUT_AOS)
        return set_err(GSR_E_ARG, "%s: GSR_LAYOUT_AOS has no gradient planes; upload a scene block", who);
    if (out->d_temporal && layout != GSR_LAYOUT_SCENE_BLOCK_4D)
        return set_err(GSR_E_ARG, "%s: d_temporal needs a 4D scene block", who);
    return GSR_OK;
}

int project_backward_launch(const gsr_context* c, const void* scene, int layout, int64_t n, const Frame& fr,
                            const gsr_record_grads& in, const gsr_scene_grads& out, hipStream_t s,
                            const float* in_z = nullptr) {
    if (n == 0) return GSR_OK;
    HIP_TRY(gsr::launch_project_backward(scene_arrays(scene), scene_stride(n), n, fr, layout == GSR_LAYOUT_SCENE_BLOCK_4D,
                                         layout == GSR_LAYOUT_SCENE_BLOCK_SH3, c->time, in, out, s, in_z));
    return GSR_OK;
}

}  // namespace

extern "C" int gsr_project_backward(gsr_context* c, const void* scene, int layout, int64_t n, const gsr_camera* cam,
                                    int W, int H, float k, const gsr_record_grads* in, const gsr_scene_grads* out,
                                    void* stream) {
    if (!c) return set_err(GSR_E_ARG, "null context");
    if (!in) return set_err(GSR_E_ARG, "gsr_project_backward: null inputs");
    if (!in->d_color && !in->d_opacity && !in->d_conic && !in->d_center)
        return set_err(GSR_E_ARG, "gsr_project_backward: no upstream gradient");
    if (int rc = check_scene_grads("gsr_project_backward", out, layout)) return rc;
    if (int rc = check_scene_args(scene, layout, n)) return rc;
    // a frame of its own: the context's (the last rendered frame's) is left alone
    Frame fr;
    if (int rc = fill_frame(fr, cam, W, H, 1, 1, W, H, k)) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    return project_backward_launch(c, scene, layout, n, fr, *in, *out, static_cast<hipStream_t>(stream));
}

extern "C" int gsr_render_backward_scene(gsr_context* c, const void* scene, int layout, int64_t n,
                                         const gsr_camera* cam, int W, int H, int nx, int ny, int ws, int hs, float k,
                                         const float* d_grad_image, const float* d_grad_alpha, float* d_scratch,
                                         const gsr_scene_grads* out, void* stream) {
    if (!c) return set_err(GSR_E_ARG, "null context");
    if (!d_grad_image && !d_grad_alpha)
        return set_err(GSR_E_ARG, "gsr_render_backward_scene: no upstream gradient");
    if (int rc = check_scene_grads("gsr_render_backward_scene", out, layout)) return rc;
    if (int rc = check_scene_args(scene, layout, n)) return rc;
    {
        Frame probe;   // the frame's argument errors, before the planes are zeroed
        if (int rc = fill_frame(probe, cam, W, H, nx, ny, ws, hs, k)) return rc;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    float* planes = d_scratch;
    if (!planes && n > 0) {
        if (int rc = c->rec_grads.reserve(10 * per_gaussian(n))) return rc;   // ten planes of n floats
        planes = c->rec_grads;
    }
    if (n > 0) HIP_TRY(hipMemsetAsync(planes, 0, 10 * (size_t)n * sizeof(float), static_cast<hipStream_t>(stream)));
    const gsr_backward_targets bw{d_grad_image, d_grad_alpha, planes, planes + 3 * n, planes + 4 * n, planes + 8 * n};
    const int rc = aux_frame_locked(c, scene, layout, n, cam, W, H, nx, ny, ws, hs, k, stream,
                                    [&] { return blend_backward_locked(c, bw); });
    if (rc != GSR_OK && rc != GSR_E_OVERFLOW) return rc;
    const gsr_record_grads in{planes, planes + 3 * n, planes + 4 * n, planes + 8 * n};
    if (int r2 = project_backward_launch(c, scene, layout, n, c->fr, in, *out, c->stream)) return r2;
    return rc;
}

// ------------------------------------------------------------------ backward with the depth and feature planes

namespace {

// What gsr_render_backward_aux and gsr_render_backward_scene_aux refuse in their upstream.
int check_aux_upstream(const char* who, const gsr_aux_upstream* up, const float* d_feat) {
    if (!up) return set_err(GSR_E_ARG, "%s: null upstream", who);
    if (up->nfeat < 0 || up->nfeat > GSR_AUX_MAX_FEATURES)
        return set_err(GSR_E_ARG, "%s: nfeat %d out of range [0, %d]", who, up->nfeat, GSR_AUX_MAX_FEATURES);
    if (up->nfeat > 0 && !up->d_features) return set_err(GSR_E_ARG, "%s: nfeat %d needs d_features", who, up->nfeat);
    if (up->nfeat == 0 && (up->d_grad_feat || d_feat))
        return set_err(GSR_E_ARG, "%s: feature gradients given with nfeat 0", who);
    if (!up->d_grad_image && !up->d_grad_alpha && !up->d_grad_depth && !up->d_grad_feat)
        return set_err(GSR_E_ARG, "%s: no upstream gradient", who);
    return GSR_OK;
}

// The sorted frame's backward pass with the depth and feature channels: blend_backward_locked
// with k_blend_backward_aux, behind blend_aux_locked's -Z kernel and workspaces where a
// channel reaches an output.  Without either channel it is blend_backward_locked.
int blend_backward_aux_locked(gsr_context* c, const gsr_aux_upstream& up, const gsr_record_grads_aux_out& o) {
    const bool geo = o.d_opacity || o.d_conic || o.d_center;
    if (!up.d_grad_depth && !up.d_grad_feat && !o.d_z && !o.d_feat) {
        // (d_color without d_grad_image is identically zero: not touched here either)
        float* color = up.d_grad_image ? o.d_color : nullptr;
        if (!color && !geo) {
            mark(c, GSR_STAGE_BLEND);
            return frame_done(c);
        }
        const gsr_backward_targets bw{up.d_grad_image, up.d_grad_alpha, color, o.d_opacity, o.d_conic, o.d_center};
        return blend_backward_locked(c, bw);
    }
    // -Z and the feature values enter through u alone, which only the geometry outputs need
    const bool with_z = up.d_grad_depth && geo && c->n > 0;
    const bool with_pack = up.nfeat > 4 && up.d_grad_feat && geo && c->n > 0;
    if (with_z) {
        if (int rc = c->aux_z.reserve(per_gaussian(c->n))) return rc;
    }
    if (with_pack) {
        if (int rc = c->aux_pack.reserve(2 * per_gaussian(c->n))) return rc;
    }
    mark(c, GSR_STAGE_BLEND);   // the stage holds the -Z and feature-pack kernels too
    if (with_z)
        HIP_TRY(gsr::launch_aux_depth(c->pre_arrays, c->pre_stride, c->n, c->fr,
                                      c->pre_layout == GSR_LAYOUT_SCENE_BLOCK_4D, c->time, c->aux_z, c->stream));
    HIP_TRY(gsr::launch_blend_backward_aux(pair_vals(c, c->pair_buf), c->ranges, c->rec, c->fr, up.d_grad_image,
                                           up.d_grad_alpha, up.d_grad_depth, up.d_grad_feat, up.d_features, up.nfeat,
                                           c->aux_z, c->aux_pack, o.d_color, o.d_opacity, o.d_conic, o.d_center,
                                           o.d_z, o.d_feat, c->n, &c->stats[0].overflow, c->set.blend_band_tiles,
                                           c->stream));
    return frame_done(c);
}

}  // namespace

extern "C" int gsr_render_backward_aux(gsr_context* c, const void* scene, int layout, int64_t n,
                                       const gsr_camera* cam, int W, int H, int nx, int ny, int ws, int hs, float k,
                                       const gsr_aux_upstream* up, const gsr_record_grads_aux_out* out,
                                       void* stream) {
    if (!c) return set_err(GSR_E_ARG, "null context");
    if (!out) return set_err(GSR_E_ARG, "gsr_render_backward_aux: null outputs");
    if (int rc = check_aux_upstream("gsr_render_backward_aux", up, out->d_feat)) return rc;
    if (!out->d_color && !out->d_opacity && !out->d_conic && !out->d_center && !out->d_z && !out->d_feat)
        return set_err(GSR_E_ARG, "gsr_render_backward_aux: no output");
    std::lock_guard<std::mutex> lk(c->mu);
    return aux_frame_locked(c, scene, layout, n, cam, W, H, nx, ny, ws, hs, k, stream,
                            [&] { return blend_backward_aux_locked(c, *up, *out); });
}

extern "C" int gsr_project_backward_aux(gsr_context* c, const void* scene, int layout, int64_t n,
                                        const gsr_camera* cam, int W, int H, float k, const gsr_record_grads_aux* in,
                                        const gsr_scene_grads* out, void* stream) {
    if (!c) return set_err(GSR_E_ARG, "null context");
    if (!in) return set_err(GSR_E_ARG, "gsr_project_backward_aux: null inputs");
    if (!in->d_color && !in->d_opacity && !in->d_conic && !in->d_center && !in->d_z)
        return set_err(GSR_E_ARG, "gsr_project_backward_aux: no upstream gradient");
    if (int rc = check_scene_grads("gsr_project_backward_aux", out, layout)) return rc;
    if (int rc = check_scene_args(scene, layout, n)) return rc;
    // a frame of its own: the context's (the last rendered frame's) is left alone
    Frame fr;
    if (int rc = fill_frame(fr, cam, W, H, 1, 1, W, H, k)) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    const gsr_record_grads ten{in->d_color, in->d_opacity, in->d_conic, in->d_center};
    return project_backward_launch(c, scene, layout, n, fr, ten, *out, static_cast<hipStream_t>(stream), in->d_z);
}

extern "C" int gsr_render_backward_scene_aux(gsr_context* c, const void* scene, int layout, int64_t n,
                                             const gsr_camera* cam, int W, int H, int nx, int ny, int ws, int hs,
                                             float k, const gsr_aux_upstream* up, float* d_feat_grad,
                                             float* d_scratch, const gsr_scene_grads* out, void* stream) {
    if (!c) return set_err(GSR_E_ARG, "null context");
    if (int rc = check_aux_upstream("gsr_render_backward_scene_aux", up, d_feat_grad)) return rc;
    if (int rc = check_scene_grads("gsr_render_backward_scene_aux", out, layout)) return rc;
    if (int rc = check_scene_args(scene, layout, n)) return rc;
    {
        Frame probe;   // the frame's argument errors, before the planes are zeroed
        if (int rc = fill_frame(probe, cam, W, H, nx, ny, ws, hs, k)) return rc;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    float* planes = d_scratch;
    if (!planes && n > 0) {
        if (int rc = c->rec_grads.reserve(11 * per_gaussian(n))) return rc;   // eleven planes of n floats
        planes = c->rec_grads;
    }
    if (n > 0) HIP_TRY(hipMemsetAsync(planes, 0, 11 * (size_t)n * sizeof(float), static_cast<hipStream_t>(stream)));
    const gsr_record_grads_aux_out rg{planes, planes + 3 * n, planes + 4 * n, planes + 8 * n, planes + 10 * n,
                                      d_feat_grad};
    const int rc = aux_frame_locked(c, scene, layout, n, cam, W, H, nx, ny, ws, hs, k, stream,
                                    [&] { return blend_backward_aux_locked(c, *up, rg); });
    if (rc != GSR_OK && rc != GSR_E_OVERFLOW) return rc;
    const gsr_record_grads in{planes, planes + 3 * n, planes + 4 * n, planes + 8 * n};
    // (without a depth gradient the z plane stays zero: the ten-entry kernel)
    const float* in_z = up->d_grad_depth ? planes + 10 * n : nullptr;
    if (int r2 = project_backward_launch(c, scene, layout, n, c->fr, in, *out, c->stream, in_z)) return r2;
    return rc;
}

// ------------------------------------------------------------------ sync

extern "C" int gsr_sync(gsr_context* c) {
    if (!c) return set_err(GSR_E_ARG, "null context");
    std::lock_guard<std::mutex> lk(c->mu);
    int result = GSR_OK;
    for (size_t l = 0; l < c->lanes.size(); l++) {
        gsr_context* lc = c->lanes[l];
        HIP_TRY(hipStreamSynchronize(c->lane_streams[l]));
        const int rc = check_overflow(lc, true);
        if (rc != GSR_OK && rc != GSR_E_OVERFLOW) return rc;
        if (lc->overflow_seen) result = GSR_E_OVERFLOW;
        lc->overflow_seen = false;
    }
    if (c->stream || c->pending) HIP_TRY(hipStreamSynchronize(c->stream));
    const int rc = check_overflow(c, true);
    if (rc != GSR_OK && rc != GSR_E_OVERFLOW) return rc;
    if (c->overflow_seen) result = GSR_E_OVERFLOW;
    c->overflow_seen = false;
    if (result == GSR_E_OVERFLOW && rc == GSR_OK)
        set_err(GSR_E_OVERFLOW, "a frame since the last gsr_sync was incomplete (reported earlier); re-render");
    return result;
}

