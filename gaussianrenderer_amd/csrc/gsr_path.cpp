// gsr_path.cpp — frames in flight: gsr_render_path and its two extended forms render a camera
// path's frames on up to GSR_MAX_FRAMES_IN_FLIGHT lanes.  Lane 0 is the caller's context on
// the caller's stream; every other lane is a private child context on a stream of its own.
#include <algorithm>
#include <unordered_map>
#include <utility>
#include <vector>

#include "gsr_context.h"

using namespace gsr;

namespace {

// What a lane inherits from lane 0: the settings; diagnostics and timing stay on lane 0 only,
// and the split point adapts per lane (set at creation and by the knob).
void copy_settings(gsr_context* d, const gsr_context* s) { d->set = s->set; }

// Lanes 1..F-1: child contexts, streams and events, created once and kept.
int ensure_lanes(gsr_context* c, int F) {
    if (!c->fork_ev) HIP_TRY(hipEventCreateWithFlags(&c->fork_ev, hipEventDisableTiming));
    if (!c->pre_ev) HIP_TRY(hipEventCreateWithFlags(&c->pre_ev, hipEventDisableTiming));
    while ((int)c->lanes.size() < F - 1) {
        gsr_context* l = new gsr_context();
        l->inflight = 1;
        l->ctl.split_pm = c->ctl.split_pm;
        l->ctl.split_floor = c->ctl.split_floor;
        hipStream_t s = nullptr;
        hipEvent_t e = nullptr;
        if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
            if (s) (void)hipStreamDestroy(s);
            gsr_destroy(l);
            return set_err(GSR_E_HIP, "frames in flight: stream/event creation failed");
        }
        c->lanes.push_back(l);
        c->lane_streams.push_back(s);
        c->join_evs.push_back(e);
    }
    while ((int)c->alias_evs.size() < F) {
        hipEvent_t e = nullptr;
        HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        c->alias_evs.push_back(e);
    }
    for (int l = 0; l < F - 1; l++) copy_settings(c->lanes[l], c);
    return GSR_OK;
}

// Shared preprocess: the lane's second set of preprocess outputs, as large as the first.
int ensure_alt(gsr_context* c) {
    if (!c->alt_ev) HIP_TRY(hipEventCreateWithFlags(&c->alt_ev, hipEventDisableTiming));
    if (c->alt_cap >= c->n_cap) return GSR_OK;
    HIP_TRY(hipDeviceSynchronize());
    if (int rc = c->alt_rec.alloc(4 * (size_t)c->n_cap)) return rc;
    if (int rc = c->alt_items.alloc((size_t)c->n_cap)) return rc;
    if (int rc = c->alt_rect.alloc((size_t)c->n_cap)) return rc;
    if (int rc = c->alt_spans.alloc((size_t)c->n_cap)) return rc;
    c->alt_cap = c->n_cap;
    return GSR_OK;
}

// The planned frame's preprocess outputs (records, the item buffer the plan chose, rects,
// spans) become the other set; the set they were stays with whatever the lane has queued.
void switch_pre_set(gsr_context* c) {
    const int b = c->pre_out == c->items[1] ? 1 : 0;
    std::swap(c->rec, c->alt_rec);
    std::swap(c->items[b], c->alt_items);
    std::swap(c->rect, c->alt_rect);
    std::swap(c->spans, c->alt_spans);
    c->pre_out = c->items[b];
}

int render_one_locked(gsr_context* c, const void* scene, int layout, int64_t n, const gsr_camera* cam, int W,
                      int H, int nx, int ny, int ws, int hs, float k, float* d_out, hipStream_t s) {
    int rc = preprocess_locked(c, scene, layout, n, cam, W, H, nx, ny, ws, hs, k, s);
    if (rc != GSR_OK && rc != GSR_E_OVERFLOW) return rc;
    if (int r2 = sort_locked(c, true)) return r2;
    if (int r3 = blend_locked(c, d_out)) return r3;
    return rc;
}

// One call of gsr_render_path_status, after its argument checks, under the context's mutex.
// Frame i runs on lane i % F; the frames are taken in groups of F, one per lane.
struct PathRun {
    gsr_context* const c;
    const hipStream_t S;             // the caller's stream: lane 0's
    const int F;                     // lanes this call uses
    const void* const scene;
    const int layout;
    const int64_t n;
    const gsr_camera* const cams;
    const float* const times;
    const int nframes, W, H, nx, ny, ws, hs;
    const float k;
    float* const* const d_outs;
    void* const* const frame_events;
    void* const* const wait_events;
    const int flags;
    uint32_t* const* const d_status;
    // Output reuse: a frame writing a buffer that an earlier frame of this call wrote on
    // ANOTHER lane must wait for that writer, however far back it ran (lanes are not
    // ordered with each other).  prev[i] = the last earlier frame writing d_outs[i];
    // a writer whose buffer is reused on another lane records its lane's event after
    // it, and the reuser waits on that event's latest record (at or after the writer
    // on the same stream, so the wait covers it).
    std::vector<int> prev;
    std::vector<char> record;
    int result = GSR_OK;             // GSR_E_OVERFLOW once a frame reported one
    int err = GSR_OK;                // the first error; the frames queued before it are still joined
    const float t_saved;             // the context's time knob, restored by join

    // the frame's validity word is the lane's only while its frame is queued: the guard
    // clears it on every exit, so a later gsr_render on this context (or an erroring
    // frame's early return) never writes through a pointer the caller may have freed
    struct StatusScope {
        gsr_context* lc;
        ~StatusScope() { lc->fstatus = nullptr; }
    };

    static int hip_fail(hipError_t e, const char* what) {
        return set_err(GSR_E_HIP, "gsr_render_path: %s: %s", what, hipGetErrorString(e));
    }
    gsr_context* lane_ctx(int lane) const { return lane == 0 ? c : c->lanes[lane - 1]; }
    hipStream_t lane_stream(int lane) const { return lane == 0 ? S : c->lane_streams[lane - 1]; }

    // what frame i's lane waits for before it renders: the earlier writer of its output
    // on another lane, and the caller's event
    int frame_waits(int i) const {
        const int lane = i % F;
        const hipStream_t ls = lane_stream(lane);
        if (prev[i] >= 0 && prev[i] % F != lane) {
            if (hipError_t e = hipStreamWaitEvent(ls, c->alias_evs[prev[i] % F], 0))
                return hip_fail(e, "output reuse wait");
        }
        if (wait_events && wait_events[i]) {
            if (hipError_t e = hipStreamWaitEvent(ls, static_cast<hipEvent_t>(wait_events[i]), 0))
                return hip_fail(e, "wait event");
        }
        return GSR_OK;
    }

    // rc: the frame's own result.  Notes an overflow, records the frame's events; returns an error
    int frame_done(int i, int rc) {
        const int lane = i % F;
        const hipStream_t ls = lane_stream(lane);
        if (rc == GSR_E_OVERFLOW) result = GSR_E_OVERFLOW;
        else if (rc != GSR_OK) return rc;
        if (record[i]) {
            if (hipError_t e = hipEventRecord(c->alias_evs[lane], ls)) return hip_fail(e, "output reuse event");
        }
        if (frame_events && frame_events[i]) {
            if (hipError_t e = hipEventRecord(static_cast<hipEvent_t>(frame_events[i]), ls))
                return hip_fail(e, "frame event");
        }
        return GSR_OK;
    }

    int fail_hook(int i) {   // GSR_TUNE_FAIL_FRAME (test hook, once)
        if (!(c->fail_frame > 0 && i == c->fail_frame)) return GSR_OK;
        c->fail_frame = 0;
        return set_err(GSR_E_ARG, "gsr_render_path: frame %d failed (GSR_TUNE_FAIL_FRAME test hook)", i);
    }

    // Lanes, static buffers, the children's pair capacity, the fork, the output-reuse table.
    // An error here returns before any lane has work of this call: no join is needed.
    int prepare() {
        if (int rc = ensure_lanes(c, F)) return rc;
        if (int rc = ensure_static(c)) return rc;
        // children start at the parent's pair high-water mark (each still grows on its own overflow)
        for (int l = 0; l < F - 1; l++) {
            gsr_context* ch = c->lanes[l];
            if (int rc = ensure_static(ch)) return rc;
            if (ch->p_cap < c->p_cap && c->p_cap > 0) {
                if (int rc = ensure_n(ch, std::max<int64_t>(n, 1))) return rc;
                if (int rc = ensure_pairs(ch, c->p_cap)) return rc;
            }
        }
        // fork: every lane starts after the work already queued on the caller's stream
        if (F > 1 && !(flags & GSR_PATH_NO_FORK)) {
            HIP_TRY(hipEventRecord(c->fork_ev, S));
            for (int l = 0; l < F - 1; l++) HIP_TRY(hipStreamWaitEvent(c->lane_streams[l], c->fork_ev, 0));
        }
        prev = std::vector<int>(nframes, -1);
        record = std::vector<char>(nframes, 0);
        std::unordered_map<const float*, int> last;
        last.reserve(2 * (size_t)nframes);
        for (int i = 0; i < nframes; i++) {
            auto it = last.find(d_outs[i]);
            if (it != last.end()) {
                prev[i] = it->second;
                if (it->second % F != i % F) record[it->second] = 1;
            }
            last[d_outs[i]] = i;
        }
        return GSR_OK;
    }

    // Host only: plans the group's frames, lane by lane, until one fails (err); returns how many
    // were planned.  A plan that fails launches nothing for its frame or any after it.
    int plan_group(int g0, int m) {
        int planned = 0;
        for (; planned < m && err == GSR_OK; planned++) {
            const int i = g0 + planned;
            gsr_context* lc = lane_ctx(planned);
            lc->time = times ? times[i] : t_saved;
            int rc = fail_hook(i);
            if (rc == GSR_OK)
                rc = preprocess_plan(lc, scene, layout, n, &cams[i], W, H, nx, ny, ws, hs, k, lane_stream(planned));
            if (rc == GSR_OK || rc == GSR_E_OVERFLOW) {
                if (rc == GSR_E_OVERFLOW) result = GSR_E_OVERFLOW;
                rc = ensure_alt(lc);
            }
            if (rc != GSR_OK) {
                err = rc;
                break;
            }
        }
        return planned;
    }

    // The preprocess of the group's `planned` >= 2 planned frames as k_preprocess_multi launches on
    // lane 0's stream (at most kPreMultiMax cameras per launch, a remainder of one by
    // k_preprocess).  Returns the first error of its steps: none of the group's frames is rendered.
    int launch_shared(int g0, int planned) {
        int perr = GSR_OK;
        auto hip_step = [&](hipError_t e, const char* what) {
            if (e != hipSuccess && perr == GSR_OK) perr = hip_fail(e, what);
        };
        // the launches overwrite each lane's other set: they wait for the work that
        // used it (everything the lane had queued when it last switched sets), and for
        // the events the caller gave the frames.  Then each lane marks the end of the
        // work on its current set and switches.
        for (int j = 0; j < planned; j++) {
            hip_step(hipStreamWaitEvent(S, lane_ctx(j)->alt_ev, 0), "shared preprocess wait");
            if (j > 0 && wait_events && wait_events[g0 + j])
                hip_step(hipStreamWaitEvent(S, static_cast<hipEvent_t>(wait_events[g0 + j]), 0), "wait event");
        }
        if (perr == GSR_OK) perr = frame_waits(g0);
        for (int j = 0; j < planned && perr == GSR_OK; j++) {
            hip_step(hipEventRecord(lane_ctx(j)->alt_ev, lane_stream(j)), "shared preprocess event");
            if (perr == GSR_OK) switch_pre_set(lane_ctx(j));
        }
        for (int j = 0; j < planned && perr == GSR_OK;) {
            const int nc = std::min(gsr::kPreMultiMax, planned - j);
            if (nc == 1) {
                if (int rc = preprocess_launch(lane_ctx(j), S)) perr = rc;
            } else {
                const gsr::Frame* frs[gsr::kPreMultiMax];
                gsr::PreTargets outs[gsr::kPreMultiMax];
                for (int q = 0; q < nc; q++) {
                    gsr_context* lc = lane_ctx(j + q);
                    frs[q] = &lc->fr;
                    outs[q] = gsr::PreTargets{lc->rec, lc->pre_out, lc->rect, lc->spans_frame ? lc->spans : nullptr,
                                              lc->rect_packed};
                }
                hip_step(gsr::launch_preprocess_multi(c->pre_arrays, c->pre_stride, n, nc, frs, outs,
                                                      layout == GSR_LAYOUT_SCENE_BLOCK_SH3, S),
                         "shared preprocess");
                for (int q = 0; q < nc && perr == GSR_OK; q++) preprocess_queued(lane_ctx(j + q));
                if (perr == GSR_OK) c->shared_launches++;
            }
            j += nc;
        }
        if (perr == GSR_OK) hip_step(hipEventRecord(c->pre_ev, S), "shared preprocess event");
        for (int j = 1; j < planned && perr == GSR_OK; j++)
            hip_step(hipStreamWaitEvent(lane_stream(j), c->pre_ev, 0), "shared preprocess wait");
        return perr;
    }

    // Shared preprocess (GSR_TUNE_PATH_SHARED_PRE): the frames of a group (one per lane) are
    // planned first, then the shared launches write every lane's preprocess outputs, and each
    // lane sorts and blends on its own stream as usual.
    void group_shared(int g0, int m) {
        const int planned = plan_group(g0, m);
        int perr = GSR_OK;
        if (planned >= 2) {
            perr = launch_shared(g0, planned);
        } else if (planned == 1) {
            perr = frame_waits(g0);
            if (perr == GSR_OK) perr = preprocess_launch(c, S);
        }
        if (perr != GSR_OK) {
            if (err == GSR_OK) err = perr;
            return;
        }
        // the frames planned before a failed plan still complete; an error of theirs is the earlier one
        for (int j = 0; j < planned; j++) {
            const int i = g0 + j;
            gsr_context* lc = lane_ctx(j);
            int rc = j > 0 ? frame_waits(i) : (int)GSR_OK;
            if (rc == GSR_OK) {
                StatusScope status_scope{lc};
                lc->fstatus = d_status ? d_status[i] : nullptr;
                rc = sort_locked(lc, true);
                if (rc == GSR_OK) rc = blend_locked(lc, d_outs[i]);
                rc = frame_done(i, rc);
            }
            if (rc != GSR_OK) {
                err = rc;
                return;
            }
        }
    }

    // Each frame of the group whole (preprocess, sort, blend) on its own lane.
    void group_plain(int g0, int m) {
        for (int i = g0; i < g0 + m && err == GSR_OK; i++) {
            const int lane = i % F;
            gsr_context* lc = lane_ctx(lane);
            if (int rc = frame_waits(i)) {
                err = rc;
                return;
            }
            lc->time = times ? times[i] : t_saved;
            StatusScope status_scope{lc};
            lc->fstatus = d_status ? d_status[i] : nullptr;
            int rc = fail_hook(i);
            if (rc == GSR_OK)
                rc = render_one_locked(lc, scene, layout, n, &cams[i], W, H, nx, ny, ws, hs, k, d_outs[i],
                                       lane_stream(lane));
            err = frame_done(i, rc);
        }
    }

    // On every exit after the fork, errors included (render.cu:914-923 reports a failed
    // step and the caller's frame loop goes on): the time knob is restored, the caller's
    // stream is the context's again, and work queued on it afterwards sees every frame the
    // lanes took (a caller that frees or reuses an output after an error must not race a
    // lane still writing it).  A join failure after an earlier error keeps the first message.
    int join() {
        c->time = t_saved;
        c->stream = S;
        for (int l = 0; l < F - 1 && l + 1 < nframes && !(flags & GSR_PATH_NO_JOIN); l++) {
            hipError_t e = hipEventRecord(c->join_evs[l], c->lane_streams[l]);
            if (e == hipSuccess) e = hipStreamWaitEvent(S, c->join_evs[l], 0);
            if (e != hipSuccess && err == GSR_OK) err = hip_fail(e, "join");
        }
        return err != GSR_OK ? err : result;
    }

    int run() {
        if (int rc = prepare()) return rc;
        const bool shared_ok = c->path_shared_pre && F >= 2 && n > 0 &&
                               (layout == GSR_LAYOUT_SCENE_BLOCK || layout == GSR_LAYOUT_SCENE_BLOCK_SH3) &&
                               !c->diagnostics && c->timing != 2;
        for (int g0 = 0; g0 < nframes && err == GSR_OK; g0 += F) {
            const int m = std::min(F, nframes - g0);
            // the depth split off on every lane of the group (a lane's controller may turn it
            // back on between groups; a plan that does so still writes the plain outputs)
            bool shared = shared_ok && m >= 2;
            for (int l = 0; l < m && shared; l++) shared = !split_enabled(lane_ctx(l), n);
            if (shared) group_shared(g0, m);
            else group_plain(g0, m);
        }
        return join();
    }
};

}  // namespace

extern "C" int gsr_set_frames_in_flight(gsr_context* c, int frames) {
    if (!c || frames < 1 || frames > GSR_MAX_FRAMES_IN_FLIGHT)
        return set_err(GSR_E_ARG, "gsr_set_frames_in_flight: frames must be 1..%d", GSR_MAX_FRAMES_IN_FLIGHT);
    std::lock_guard<std::mutex> lk(c->mu);
    c->inflight = frames;
    return GSR_OK;
}

extern "C" int gsr_frames_in_flight(gsr_context* c) {
    if (!c) return set_err(GSR_E_ARG, "null context");
    return c->inflight;
}

extern "C" int gsr_render_path(gsr_context* c, const void* scene, int layout, int64_t n, const gsr_camera* cams,
                               const float* times, int nframes, int W, int H, int nx, int ny, int ws, int hs,
                               float k, float* const* d_outs, void* stream) {
    return gsr_render_path_ex(c, scene, layout, n, cams, times, nframes, W, H, nx, ny, ws, hs, k, d_outs, stream,
                              nullptr, nullptr, 0);
}

extern "C" int gsr_render_path_ex(gsr_context* c, const void* scene, int layout, int64_t n, const gsr_camera* cams,
                                  const float* times, int nframes, int W, int H, int nx, int ny, int ws, int hs,
                                  float k, float* const* d_outs, void* stream, void* const* frame_events,
                                  void* const* wait_events, int flags) {
    return gsr_render_path_status(c, scene, layout, n, cams, times, nframes, W, H, nx, ny, ws, hs, k, d_outs, stream,
                                  frame_events, wait_events, flags, nullptr);
}

extern "C" int gsr_render_path_status(gsr_context* c, const void* scene, int layout, int64_t n,
                                      const gsr_camera* cams, const float* times, int nframes, int W, int H, int nx,
                                      int ny, int ws, int hs, float k, float* const* d_outs, void* stream,
                                      void* const* frame_events, void* const* wait_events, int flags,
                                      uint32_t* const* d_status) {
    if (!c) return set_err(GSR_E_ARG, "null context");
    if (flags & ~(GSR_PATH_NO_JOIN | GSR_PATH_NO_FORK))
        return set_err(GSR_E_ARG, "gsr_render_path_ex: unknown flags 0x%x", flags);
    if (nframes < 0 || (nframes > 0 && (!cams || !d_outs)))
        return set_err(GSR_E_ARG, "gsr_render_path: bad frame arrays");
    for (int i = 0; i < nframes; i++)
        if (!d_outs[i]) return set_err(GSR_E_ARG, "gsr_render_path: null output for frame %d", i);
    std::lock_guard<std::mutex> lk(c->mu);
    if (nframes == 0) return GSR_OK;
    PathRun run{c, static_cast<hipStream_t>(stream), std::max(1, std::min(c->inflight, nframes)), scene, layout, n,
                cams, times, nframes, W, H, nx, ny, ws, hs, k, d_outs, frame_events, wait_events, flags, d_status,
                {}, {}, GSR_OK, GSR_OK, c->time};
    return run.run();
}
