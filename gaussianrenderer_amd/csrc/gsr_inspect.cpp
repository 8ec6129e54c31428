// gsr_inspect.cpp — what reads a context back or configures it (readback of a frame's stages,
// stage timing, the tuning knobs, the blend diagnostics), and the device probes, which need no
// context at all.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "gsr_context.h"
#include "gsr_detmath.h"

using namespace gsr;

// ------------------------------------------------------------------ readback

extern "C" int64_t gsr_pair_count(gsr_context* c) {
    if (!c || !c->stats) return -1;
    std::lock_guard<std::mutex> lk(c->mu);
    Stats s{};
    if (hipStreamSynchronize(c->stream) != hipSuccess) return -1;
    if (hipMemcpy(&s, c->stats, sizeof s, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return (int64_t)s.pairs_total;
}

extern "C" int64_t gsr_row_item_count(gsr_context* c) {
    if (!c || !c->binmeta) return -1;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->have_sort || !c->last_binned) return -1;
    uint32_t rows[256];
    if (hipStreamSynchronize(c->stream) != hipSuccess) return -1;
    if (hipMemcpy(rows, c->binmeta + 256, sizeof rows, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    int64_t total = 0;
    for (uint32_t v : rows) total += v;
    return total;
}

static int depth_passes_locked(gsr_context* c, int* passes);
static int sorted_items_locked(gsr_context* c, uint64_t* host, int64_t n);

// The device record's fourth word is the blend's cull word (gsr_kernels.hip
// cull_word); the readback layout's fourth word {tile x range, tile y range,
// tile count, depth key} is rebuilt from the preprocess tile rects (index order)
// and the frame's depth items: (key << 32 | index) in index order right after
// preprocess or in a per-tile-order frame, depth-sorted after a global sort.
extern "C" int gsr_read_splats(gsr_context* c, void* host, int64_t n) {
    if (!c || !host || n < 0 || n > c->n) return set_err(GSR_E_ARG, "gsr_read_splats: bad argument");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (!n) return GSR_OK;
    if (!c->have_pre) return set_err(GSR_E_ARG, "gsr_read_splats: no preprocessed frame");
    if (c->records_partial) {   // key-mode split frame: the far Gaussians' records first
        if (int rc = far_records_locked(c, false)) return rc;
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    HIP_TRY(hipMemcpy(host, c->rec, (size_t)n * GSR_SPLAT_RECORD_BYTES, hipMemcpyDeviceToHost));
    std::vector<uint64_t> rect((size_t)n), items((size_t)c->n);
    if (c->rect_packed) {   // 4-B rects (gsr_geom_device.h pack_rect): tx0 | tx1 << 8 | ty0 << 16 | ty1 << 24
        std::vector<uint32_t> p((size_t)n);
        HIP_TRY(hipMemcpy(p.data(), c->rect, (size_t)n * 4, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < (size_t)n; i++)
            rect[i] = (uint64_t)(p[i] & 0xffu) | ((uint64_t)((p[i] >> 8) & 0xffu) << 16) |
                      ((uint64_t)((p[i] >> 16) & 0xffu) << 32) | ((uint64_t)(p[i] >> 24) << 48);
    } else {
        HIP_TRY(hipMemcpy(rect.data(), c->rect, (size_t)n * 8, hipMemcpyDeviceToHost));
    }
    if (c->have_sort && c->last_split_key) {
        // a key-mode split frame: its preprocess order holds every item's key
        HIP_TRY(hipMemcpy(items.data(), c->src_items, (size_t)c->n * 8, hipMemcpyDeviceToHost));
    } else if (c->have_sort) {
        if (int rc = sorted_items_locked(c, items.data(), c->n)) return rc;
    } else {   // preprocess order (items[1] for the live partition, src_items for a key-mode split)
        HIP_TRY(hipMemcpy(items.data(), c->pre_out ? c->pre_out : c->items[0], (size_t)c->n * 8,
                          hipMemcpyDeviceToHost));
    }
    auto* w = static_cast<uint32_t*>(host);
    for (uint64_t it : items) {
        const uint32_t i = (uint32_t)it;
        if (i < (uint64_t)n) w[(size_t)i * 16 + 15] = (uint32_t)(it >> 32);
    }
    for (int64_t i = 0; i < n; i++) {
        const uint64_t r = rect[(size_t)i];
        const int tx0 = (int)(r & 0xffffu), tx1 = (int)((r >> 16) & 0xffffu);
        const int ty0 = (int)((r >> 32) & 0xffffu), ty1 = (int)(r >> 48);
        uint32_t* q = w + (size_t)i * 16;
        // the device keeps the centre pixel as the float the blend uses; the
        // readback layout's int32 (exact for |px| <= 2^24, saturating like gsr_f2i_sat)
        for (int k = 8; k < 10; k++) {
            float f;
            std::memcpy(&f, q + k, 4);
            const int32_t v = f >= 2147483648.0f ? INT32_MAX : (f < -2147483648.0f ? INT32_MIN : (int32_t)f);
            std::memcpy(q + k, &v, 4);
        }
        q[12] = (uint32_t)r;
        q[13] = (uint32_t)(r >> 32);
        q[14] = (uint32_t)((tx1 - tx0 + 1) * (ty1 - ty0 + 1));
    }
    return GSR_OK;
}

static int depth_passes_locked(gsr_context* c, int* passes) {
    *passes = 4;
    if (c->last_bds) {   // bucket-sorted: no LSD passes, the order is in items[0]
        *passes = 0;
        return GSR_OK;
    }
    if (!c->set.depth_skip) return GSR_OK;
    uint32_t st[4];   // same plan as the kernels (gsr_device.h depth_pass_skipped)
    HIP_TRY(hipMemcpy(st, c->dstats, sizeof st, hipMemcpyDeviceToHost));
    int p = 1;
    for (; p < 4; ++p) {
        const bool skip = st[3] == 0u || ((~st[0] >> (8 * p)) == (st[1] >> (8 * p)) && !((st[2] >> p) & 1u));
        if (skip) break;
    }
    *passes = p;
    return GSR_OK;
}

// First n items of the last globally sorted frame's depth order (stream drained).
static int sorted_items_locked(gsr_context* c, uint64_t* host, int64_t n) {
    if (c->last_split_key)
        return set_err(GSR_E_ARG, "depth order unavailable: the last frame was depth-split by a threshold (its far "
                                  "part is sorted only when phase B runs); set GSR_TUNE_DEPTH_SPLIT to 0");
    int p = 4;
    if (int rc = depth_passes_locked(c, &p)) return rc;
    int64_t head = n;
    if (c->last_compact) {   // sorted visible prefix in items[p & 1], culled tail (index order) in items[0]
        uint32_t live = 0;
        HIP_TRY(hipMemcpy(&live, c->nlive, sizeof live, hipMemcpyDeviceToHost));
        head = std::min<int64_t>(n, live);
        if (n > head)
            HIP_TRY(hipMemcpy(host + head, c->items[0] + head, (size_t)(n - head) * 8, hipMemcpyDeviceToHost));
    }
    if (head) HIP_TRY(hipMemcpy(host, c->items[p & 1], (size_t)head * 8, hipMemcpyDeviceToHost));
    return GSR_OK;
}

extern "C" int gsr_depth_passes(gsr_context* c) {
    if (!c || !c->have_sort) return set_err(GSR_E_ARG, "gsr_depth_passes: no sorted frame");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipStreamSynchronize(c->stream));
    int p = 4;
    if (int rc = depth_passes_locked(c, &p)) return rc;
    return p;
}

extern "C" int gsr_bucket_sizes(gsr_context* c, uint32_t* sizes, int cap) {
    if (!c || cap < 0 || (cap > 0 && !sizes)) return set_err(GSR_E_ARG, "gsr_bucket_sizes: bad argument");
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->have_sort || !c->last_bds || !c->bkt_B || !c->totals) return 0;
    HIP_TRY(hipStreamSynchronize(c->stream));
    // k_bkt_scan's bucket totals (totals[0 .. B)), which a bucket-sorted frame's later
    // kernels only read
    const int m = std::min(cap, c->bkt_B);
    if (m) HIP_TRY(hipMemcpy(sizes, c->totals, (size_t)m * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return c->bkt_B;
}

extern "C" int gsr_read_depth_order(gsr_context* c, uint64_t* host, int64_t n) {
    if (!c || !host || n < 0 || n > c->n || !c->have_sort) return set_err(GSR_E_ARG, "gsr_read_depth_order: bad argument");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipStreamSynchronize(c->stream));
    return sorted_items_locked(c, host, n);
}

extern "C" int64_t gsr_read_pairs(gsr_context* c, uint64_t* host, int64_t cap) {
    if (!c || !host || cap < 0 || !c->have_sort) return set_err(GSR_E_ARG, "gsr_read_pairs: bad argument");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipStreamSynchronize(c->stream));
    Stats s{};
    HIP_TRY(hipMemcpy(&s, c->stats, sizeof s, hipMemcpyDeviceToHost));
    const int64_t m = std::min<int64_t>(cap, s.pairs_eff);
    if (!m) return 0;
    // the sorted pairs live as values + tile ranges; rebuild (tile << 32 | index) tile by
    // tile.  Ranges ascend with the tile; with tile row spans the binning leaves unused
    // slots between rows (pairs_total counts every tile of every rect), so the listed
    // pairs are packed here and their count returned.
    std::vector<uint32_t> vals((size_t)m);
    std::vector<uint2> rg((size_t)c->ntiles);
    HIP_TRY(hipMemcpy(vals.data(), pair_vals(c, c->pair_buf), (size_t)m * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(rg.data(), c->ranges, sizeof(uint2) * rg.size(), hipMemcpyDeviceToHost));
    int64_t k = 0;
    for (int t = 0; t < c->ntiles; t++) {
        if (!rg[t].y) continue;
        for (int64_t j = ~rg[t].x; j < (int64_t)rg[t].y && j < m; j++)
            host[k++] = ((uint64_t)(uint32_t)t << 32) | vals[(size_t)j];
    }
    return k;
}

extern "C" int gsr_tile_grid(gsr_context* c, int* tx, int* ty) {
    if (!c || !tx || !ty) return set_err(GSR_E_ARG, "gsr_tile_grid: bad argument");
    *tx = c->fr.tiles_x;
    *ty = c->fr.tiles_y;
    return GSR_OK;
}

extern "C" int gsr_read_tile_ranges(gsr_context* c, uint32_t* host, int64_t nt) {
    if (!c || !host || nt < 0 || nt > c->ntiles || !c->have_sort) return set_err(GSR_E_ARG, "gsr_read_tile_ranges: bad argument");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (nt) HIP_TRY(hipMemcpy(host, c->ranges, (size_t)nt * 8, hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < nt; i++) {         // device form {~start, end}, zero = empty
        const uint32_t x = host[2 * i], y = host[2 * i + 1];
        host[2 * i] = y ? ~x : 0u;
        host[2 * i + 1] = y;
    }
    return GSR_OK;
}

// ------------------------------------------------------------------ timing, the diagnostics switch, the frame time

extern "C" int gsr_set_timing(gsr_context* c, int mode) {
    return gsr_set_timing_stride(c, mode, 1);
}

extern "C" int gsr_set_timing_stride(gsr_context* c, int mode, int stride) {
    if (!c || mode < 0 || mode > 2 || stride < 1) return set_err(GSR_E_ARG, "gsr_set_timing: bad argument");
    std::lock_guard<std::mutex> lk(c->mu);
    c->timing = mode;
    c->timing_stride = stride;
    c->timing_count = 0;
    return GSR_OK;
}

extern "C" int gsr_stage_times(gsr_context* c, double* ms, int64_t* frames) {
    if (!c || !ms) return set_err(GSR_E_ARG, "gsr_stage_times: bad argument");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int s = 0; s < GSR_NUM_STAGES; s++) ms[s] = 0.0;
    for (auto& f : c->ev_frames) {
        // stages may be recorded out of index order (per-tile depth order runs its
        // depth stage after the binning passes): each stage lasts until the next
        // recorded boundary in TIME order
        hipEvent_t e0 = nullptr;
        for (int s = 0; s <= GSR_NUM_STAGES && !e0; s++) e0 = f.ev[s];
        float at[GSR_NUM_STAGES + 1];
        for (int s = 0; s <= GSR_NUM_STAGES; s++) {
            at[s] = -1.0f;
            if (f.ev[s] && e0 && hipEventElapsedTime(&at[s], e0, f.ev[s]) != hipSuccess) at[s] = -1.0f;
        }
        for (int s = 0; s < GSR_NUM_STAGES; s++) {
            if (!f.ev[s] || at[s] < 0.0f) continue;
            float next = -1.0f;
            for (int q = 0; q <= GSR_NUM_STAGES; q++)
                if (q != s && f.ev[q] && at[q] >= 0.0f && (at[q] > at[s] || (at[q] == at[s] && q > s)) &&
                    (next < 0.0f || at[q] < next))
                    next = at[q];
            if (next >= 0.0f) ms[s] += next - at[s];
        }
        for (auto e : f.ev)
            if (e) c->ev_pool.push_back(e);
    }
    if (frames) *frames = (int64_t)c->ev_frames.size();
    c->ev_frames.clear();
    return GSR_OK;
}

extern "C" int gsr_set_diagnostics(gsr_context* c, int on) {
    if (!c) return set_err(GSR_E_ARG, "null context");
    std::lock_guard<std::mutex> lk(c->mu);
    c->diagnostics = on != 0;
    return GSR_OK;
}

extern "C" int gsr_set_time(gsr_context* c, float t) {
    if (!c) return set_err(GSR_E_ARG, "null context");
    std::lock_guard<std::mutex> lk(c->mu);
    c->time = t;
    return GSR_OK;
}

// ------------------------------------------------------------------ tuning knobs

namespace {

// One row per knob that is a stored value: where it lives (a Settings field, which lanes
// inherit, or a field of the context, which is lane 0's alone), the values gsr_set_tuning
// accepts, and what it says when it refuses one.  The read-only knobs, the split point and
// GSR_TUNE_RANK_ATOMIC's read are spelled out in the two functions below.
struct Knob {
    enum Accept { kOneOf, kRange, kBool };   // v[0 .. nv) | v[0] .. v[1] inclusive | any, stored as != 0
    int id;
    int Settings::*set;
    int gsr_context::*ctx;
    Accept accept;
    int nv;
    int v[4];
    const char* refusal;

    int& at(gsr_context* c) const { return set ? c->set.*set : c->*ctx; }
    bool accepts(int x) const {
        if (accept == kRange) return x >= v[0] && x <= v[1];
        return accept == kBool || std::find(v, v + nv, x) != v + nv;
    }
};

constexpr const char* kBinItemsMsg = "binning items per thread must be 4, 8 or 16";
constexpr Knob kKnobs[] = {
    {GSR_TUNE_BLEND_SCHEDULE, nullptr, &gsr_context::blend_variant, Knob::kOneOf, 2, {0, 3},
     "blend schedule must be 0 (default) or 3 (timeline stamps)"},
    {GSR_TUNE_TILE_SORT_ITEMS, &Settings::tile_items, nullptr, Knob::kOneOf, 2, {8, 16},
     "tile-sort items must be 8 or 16"},
    {GSR_TUNE_DEPTH_SORT_ITEMS, &Settings::depth_items, nullptr, Knob::kOneOf, 4, {0, 4, 8, 16},
     "depth-sort items must be 0, 4, 8 or 16"},
    {GSR_TUNE_TILE_SORT_GROUPS, &Settings::tile_groups, nullptr, Knob::kRange, 2, {0, gsr::kMaxSortGroups},
     "bad group cap"},
    {GSR_TUNE_DEPTH_SORT_GROUPS, &Settings::depth_groups, nullptr, Knob::kRange, 2, {0, gsr::kMaxSortGroups},
     "bad group cap"},
    {GSR_TUNE_TILE_SORT_SPLIT, &Settings::tile_split_even, nullptr, Knob::kBool, 0, {}, nullptr},
    {GSR_TUNE_DEPTH_SORT_SKIP, &Settings::depth_skip, nullptr, Knob::kBool, 0, {}, nullptr},
    {GSR_TUNE_TILE_BINNING, &Settings::tile_binning, nullptr, Knob::kBool, 0, {}, nullptr},
    {GSR_TUNE_BIN_ROW_ITEMS, &Settings::bin_row_items, nullptr, Knob::kOneOf, 3, {4, 8, 16}, kBinItemsMsg},
    {GSR_TUNE_BIN_COL_ITEMS, &Settings::bin_col_items, nullptr, Knob::kOneOf, 3, {4, 8, 16}, kBinItemsMsg},
    {GSR_TUNE_BIN_COL_GROUPS, &Settings::bin_col_groups, nullptr, Knob::kRange, 2, {0, 65536},
     "bad column-pass group count"},
    {GSR_TUNE_COMPLETION_EVENTS, &Settings::completion_events, nullptr, Knob::kBool, 0, {}, nullptr},
    {GSR_TUNE_BLEND_BAND_TILES, &Settings::blend_band_tiles, nullptr, Knob::kRange, 2, {0, 65536},
     "blend band tiles must be 0..65536"},
    {GSR_TUNE_DEPTH_COMPACT, &Settings::depth_compact, nullptr, Knob::kRange, 2, {0, 2},
     "depth compaction must be 0, 1 or 2"},
    {GSR_TUNE_TILE_SPANS, &Settings::tile_spans, nullptr, Knob::kRange, 2, {0, 2}, "tile spans must be 0, 1 or 2"},
    {GSR_TUNE_RANK_ATOMIC, &Settings::rank_atomic, nullptr, Knob::kRange, 2, {0, 1}, "rank path must be 0 or 1"},
    {GSR_TUNE_BLEND_EXP, &Settings::blend_exp, nullptr, Knob::kRange, 2, {0, 2}, "blend exp must be 0, 1 or 2"},
    {GSR_TUNE_DEPTH_SPLIT, &Settings::depth_split, nullptr, Knob::kRange, 2, {0, 2}, "depth split must be 0, 1 or 2"},
    {GSR_TUNE_DEPTH_BUCKETS, &Settings::bucket_sort, nullptr, Knob::kRange, 2, {0, 3}, "depth buckets must be 0..3"},
    {GSR_TUNE_BUCKET_ROWS, &Settings::fuse_rows, nullptr, Knob::kBool, 0, {}, nullptr},
    {GSR_TUNE_COL_CHUNK, &Settings::col_chunk, nullptr, Knob::kOneOf, 3, {0, 1024, 2048},
     "column chunk must be 0, 1024 or 2048"},
    {GSR_TUNE_FAIL_FRAME, nullptr, &gsr_context::fail_frame, Knob::kRange, 2, {0, INT32_MAX},
     "fail frame must be >= 0"},
    {GSR_TUNE_PATH_SHARED_PRE, nullptr, &gsr_context::path_shared_pre, Knob::kRange, 2, {0, 1},
     "shared preprocess must be 0 or 1"},
};

const Knob* find_knob(int id) {
    for (const Knob& k : kKnobs)
        if (k.id == id) return &k;
    return nullptr;
}

}  // namespace

extern "C" int gsr_get_tuning(gsr_context* c, int knob, int* value) {
    if (!c || !value) return set_err(GSR_E_ARG, "gsr_get_tuning: null argument");
    std::lock_guard<std::mutex> lk(c->mu);
    switch (knob) {   // the knobs that are not a stored value read as it stands
    case GSR_TUNE_DEPTH_SPLIT_PERMILLE: *value = c->ctl.split_pm; return GSR_OK;
    case GSR_TUNE_DEPTH_SPLIT_UNSAT:
        *value = c->hstats ? (int)((const volatile Stats*)c->hstats)->split_unsat : 0;
        return GSR_OK;
    case GSR_TUNE_DEPTH_SPLIT_STATE: *value = split_state(c); return GSR_OK;
    case GSR_TUNE_PATH_SHARED_LAUNCHES: *value = (int)std::min<int64_t>(c->shared_launches, INT32_MAX); return GSR_OK;
    case GSR_TUNE_DEPTH_BUCKETS_OVER:
    case GSR_TUNE_DEPTH_BUCKETS_WORK: {
        auto get = [&](const gsr_context* x) -> int64_t {
            if (!x->hstats) return 0;
            const volatile Stats* h = (const volatile Stats*)x->hstats;
            return knob == GSR_TUNE_DEPTH_BUCKETS_OVER ? (int64_t)h->bkt_over : (int64_t)h->bkt_over_work;
        };
        int64_t v = get(c);
        for (auto* l : c->lanes) v += get(l);
        *value = (int)std::min<int64_t>(v, INT32_MAX);
        return GSR_OK;
    }
    case GSR_TUNE_RANK_ATOMIC:   // not yet set: the environment's default
        *value = c->set.rank_atomic < 0 ? default_rank_atomic() : c->set.rank_atomic;
        return GSR_OK;
    case GSR_TUNE_RANK_ATOMIC_ACTIVE: {
        RankCheck rk;
        if (int rc = rank_check_device(&rk)) return rc;
        const int asked = c->set.rank_atomic < 0 ? default_rank_atomic() : c->set.rank_atomic;
        *value = asked > 0 && rk.state == 1 ? 1 : 0;
        return GSR_OK;
    }
    }
    const Knob* k = find_knob(knob);
    if (!k) return set_err(GSR_E_ARG, "gsr_get_tuning: unknown knob");
    *value = k->at(c);
    return GSR_OK;
}

extern "C" int gsr_set_tuning(gsr_context* c, int knob, int value) {
    if (!c) return set_err(GSR_E_ARG, "null context");
    std::lock_guard<std::mutex> lk(c->mu);
    switch (knob) {
    case GSR_TUNE_RANK_ATOMIC_ACTIVE:
    case GSR_TUNE_DEPTH_SPLIT_UNSAT:
    case GSR_TUNE_DEPTH_SPLIT_STATE:
    case GSR_TUNE_DEPTH_BUCKETS_OVER:
    case GSR_TUNE_DEPTH_BUCKETS_WORK:
    case GSR_TUNE_PATH_SHARED_LAUNCHES:
        return set_err(GSR_E_ARG, "gsr_set_tuning: knob %d is read-only", knob);
    case GSR_TUNE_DEPTH_SPLIT_PERMILLE: {
        if (value < 1 || value > 999) return set_err(GSR_E_ARG, "gsr_set_tuning: split point must be 1..999");
        auto restart = [value](gsr_context* x) {   // a new starting point for every lane, no speculation
            split_restart(x, value);
            x->ctl.split_spec = false;
        };
        restart(c);
        for (auto* l : c->lanes) restart(l);
        return GSR_OK;
    }
    }
    const Knob* k = find_knob(knob);
    if (!k) return set_err(GSR_E_ARG, "gsr_set_tuning: unknown knob");
    if (!k->accepts(value)) return set_err(GSR_E_ARG, "gsr_set_tuning: %s", k->refusal);
    k->at(c) = k->accept == Knob::kBool ? value != 0 : value;
    if (knob == GSR_TUNE_DEPTH_SPLIT) {
        // the next split frame sorts the whole order (count mode), queues phase B
        c->ctl.split_key_ready = c->ctl.split_spec = false;
        for (auto* l : c->lanes) l->ctl.split_key_ready = l->ctl.split_spec = false;
    }
    return GSR_OK;
}

// ------------------------------------------------------------------ blend variant, counters, stamps, take map

extern "C" int gsr_set_blend_variant(gsr_context* c, int variant) {
    if (!c) return set_err(GSR_E_ARG, "null context");
    if (variant != 0 && variant != 3)
        return set_err(GSR_E_ARG, "gsr_set_blend_variant: variant must be 0 (default) or 3 (timeline stamps)");
    std::lock_guard<std::mutex> lk(c->mu);
    c->blend_variant = variant;
    return GSR_OK;
}

extern "C" int gsr_blend_stamps(gsr_context* c, uint64_t* out, int64_t n) {
    if (!c || !out || !c->consumed || n < 0 || n > (int64_t)c->consumed.capacity())
        return set_err(GSR_E_ARG, "gsr_blend_stamps: bad argument");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (n) HIP_TRY(hipMemcpy(out, c->consumed, (size_t)n * 8, hipMemcpyDeviceToHost));
    return GSR_OK;
}

extern "C" int64_t gsr_blend_records_loaded(gsr_context* c) {
    int64_t v[8];
    if (gsr_blend_counters(c, v)) return -1;
    return v[0];
}

extern "C" int gsr_blend_counters_ex(gsr_context* c, int64_t* out, int n) {
    if (!c || !c->consumed || !out || n < 0 || n > 16 || c->blend_variant == 3)
        return set_err(GSR_E_ARG, "gsr_blend_counters_ex: diagnostics were off or bad count");
    std::lock_guard<std::mutex> lk(c->mu);
    unsigned long long v[16] = {};
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(v, c->consumed, sizeof v, hipMemcpyDeviceToHost));
    for (int i = 0; i < n; i++) out[i] = (int64_t)v[i];
    return GSR_OK;
}

extern "C" int gsr_blend_take_map(gsr_context* c, uint64_t* out, int64_t n) {
    if (!c || !c->consumed || !out || c->blend_variant == 3 || n != (int64_t)c->fr.W * c->fr.H ||
        (int64_t)c->consumed.capacity() < 16 + n)
        return set_err(GSR_E_ARG, "gsr_blend_take_map: diagnostics were off or bad size");
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (n) HIP_TRY(hipMemcpy(out, c->consumed + 16, (size_t)n * 8, hipMemcpyDeviceToHost));
    return GSR_OK;
}

extern "C" int gsr_blend_counters(gsr_context* c, int64_t* out4) {
    if (!c || !c->consumed || !out4) return set_err(GSR_E_ARG, "gsr_blend_counters: diagnostics were off");
    std::lock_guard<std::mutex> lk(c->mu);
    unsigned long long v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(v, c->consumed, sizeof v, hipMemcpyDeviceToHost));
    for (int i = 0; i < 8; i++) out4[i] = (int64_t)v[i];
    return GSR_OK;
}

// ------------------------------------------------------------------ device probes (no context)

extern "C" int gsr_math_probe(const float* host_in, int n, float* host_out) {
    if (!host_in || !host_out || n <= 0) return set_err(GSR_E_ARG, "gsr_math_probe: bad argument");
    DevBuf<float> din, dout;
    if (int rc = din.alloc(2 * (size_t)n)) return rc;
    if (int rc = dout.alloc(9 * (size_t)n)) return rc;
    HIP_TRY(hipMemcpy(din, host_in, sizeof(float) * 2 * (size_t)n, hipMemcpyHostToDevice));
    HIP_TRY(gsr::launch_math_probe(din, n, dout, nullptr));
    HIP_TRY(hipMemcpy(host_out, dout, sizeof(float) * 9 * (size_t)n, hipMemcpyDeviceToHost));
    return GSR_OK;
}

extern "C" int gsr_exp_probe2(float x_lo, float x_hi, float x_big, int64_t* violations,
                              int64_t* packed_mismatches, float* err_all, float* err_big) {
    if (!violations || !packed_mismatches || !err_all || !err_big || !(x_lo < x_hi))
        return set_err(GSR_E_ARG, "gsr_exp_probe: bad argument");
    DevBuf<unsigned long long> dv;
    DevBuf<uint32_t> de;
    if (int rc = dv.alloc(2)) return rc;
    if (int rc = de.alloc(2)) return rc;
    HIP_TRY(hipMemset(dv, 0, 2 * sizeof(unsigned long long)));
    HIP_TRY(hipMemset(de, 0, 2 * sizeof(uint32_t)));
    HIP_TRY(gsr::launch_exp_probe(gsr_float_key(x_lo), gsr_float_key(x_hi), x_big, dv, de, nullptr));
    unsigned long long v[2] = {0, 0};
    uint32_t e[2] = {0, 0};
    HIP_TRY(hipMemcpy(v, dv, sizeof v, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(e, de, sizeof e, hipMemcpyDeviceToHost));
    *violations = (int64_t)v[0];
    *packed_mismatches = (int64_t)v[1];
    *err_all = gsr_bits_to_float(e[0]);
    *err_big = gsr_bits_to_float(e[1]);
    return GSR_OK;
}

// The round-3 signature: one int64 behind `violations` (the packed-loop count is
// gsr_exp_probe2's).
extern "C" int gsr_exp_probe(float x_lo, float x_hi, float x_big, int64_t* violations, float* err_all,
                             float* err_big) {
    int64_t packed = 0;
    return gsr_exp_probe2(x_lo, x_hi, x_big, violations, &packed, err_all, err_big);
}

extern "C" int gsr_alpha_cut_probe(const float* host_op, int n, float* host_out) {
    if (!host_op || !host_out || n <= 0) return set_err(GSR_E_ARG, "gsr_alpha_cut_probe: bad argument");
    DevBuf<float> din, dout;
    if (int rc = din.alloc((size_t)n)) return rc;
    if (int rc = dout.alloc((size_t)n)) return rc;
    HIP_TRY(hipMemcpy(din, host_op, sizeof(float) * (size_t)n, hipMemcpyHostToDevice));
    HIP_TRY(gsr::launch_xs_probe(din, n, dout, nullptr));
    HIP_TRY(hipMemcpy(host_out, dout, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost));
    return GSR_OK;
}

extern "C" int gsr_rank_order_check(int64_t* lane_ops, int64_t* mismatches) {
    if (!lane_ops || !mismatches) return set_err(GSR_E_ARG, "gsr_rank_order_check: null argument");
    unsigned long long ops = 0, bad = 0;
    HIP_TRY(gsr::rank_order_check(&ops, &bad));
    *lane_ops = (int64_t)ops;
    *mismatches = (int64_t)bad;
    return GSR_OK;
}
