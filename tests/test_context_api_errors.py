"""Every argument error of the context-bound API (gsr_create's contexts: the stage API, the frame
calls, the camera path, readback, timing, the blend diagnostics, the probes and the drop-in frame
call): what each call returns and the exact text gsr_last_error then holds, out of one table, in the
style of tests/test_scene_api_errors.py.  Rows with two bad arguments at once pin the order of the
checks; the rows without a text are the successes (and the -1 counts) that need no device and leave
the text alone.  Host code only: a context exists without a device, every row returns before any
device work, each row gets a fresh context, and the "device" pointers are addresses inside one host
buffer that must stay untouched.

Left out: messages that carry a source file and line (a failed HIP call); every row that would reach
the device (a good gsr_render, gsr_reserve, gsr_stage_times, a probe with good arguments, ...: the
GPU tests compare those); the values of gsr_get_tuning / gsr_set_tuning (tests/test_tuning_table.py);
the camera helpers, gsr_version and gsr_device_available (nothing to refuse) and the two reference
sort entry points (they return on a bad argument without a gsr_last_error text).  A fresh context has
no sorted frame and no diagnostics buffer, so gsr_read_depth_order, gsr_read_pairs,
gsr_read_tile_ranges, gsr_depth_passes and the blend counter calls have no passing row here: their
DEFAULTS are the arguments that pass once a frame exists."""
import ctypes

import pytest

INT32_MAX = 2 ** 31 - 1
BIG = INT32_MAX + 1
E = -1                                # GSR_E_ARG (include/gsr.h)


class P:
    """An address inside the host buffer: its base + off."""

    def __init__(self, off):
        self.off = off


class S:
    """A struct of _native passed by reference; a field may be a P."""

    def __init__(self, ctype, **fields):
        self.ctype, self.fields = ctype, fields


class A:
    """An array of pointers (gsr_render_path's d_outs)."""

    def __init__(self, *items):
        self.items = items


CTX = object()        # a fresh context, destroyed after the row
CAMS = object()       # two cameras (gsr_render_path's cams)
CAM_VALUE = object()  # a camera passed by value (preprocessCUDAGaussians)
INT_OUT = object()    # a fresh int holding -7
I64_OUT = object()    # a fresh int64 holding -7


def cam():
    return S("Camera", fovY=50.0, aspectRatio=1.0, nearClip=0.1, farClip=100.0)


def aux(**over):
    f = dict(d_alpha=P(8192), d_depth=None, d_features=None, nfeat=0, d_feat_out=None)
    f.update(over)
    return S("AuxTargets", **f)


def contrib(**over):
    f = dict(d_count=P(8192), d_weight=None, d_max=None, d_id=None)
    f.update(over)
    return S("ContribTargets", **f)


def backward(**over):
    f = dict(d_grad_image=P(8192), d_grad_alpha=None, d_color=P(12288), d_opacity=None, d_conic=None, d_center=None)
    f.update(over)
    return S("BackwardTargets", **f)


def rec_grads(**over):
    f = dict(d_color=P(8192), d_opacity=None, d_conic=None, d_center=None)
    f.update(over)
    return S("RecordGrads", **f)


def scene_grads(**over):
    f = dict(d_position=P(16384), d_opacity=None, d_scale=None, d_rot=None, d_sh=None, d_temporal=None)
    f.update(over)
    return S("SceneGrads", **f)


NO_GRADS = dict(d_position=None)

# a frame's arguments as gsr_preprocess takes them
FRAME = dict(scene=P(0), layout=0, n=8, cam=cam(), W=8, H=8, nx=1, ny=1, ws=8, hs=8, k=3.0)
PATH = dict(c=CTX, scene=P(0), layout=0, n=8, cams=CAMS, times=None, nframes=2, W=8, H=8, nx=1, ny=1, ws=8, hs=8,
            k=3.0, outs=A(P(4096), P(6144)), stream=None)

# call: its arguments in order, each with a value that passes every argument check
DEFAULTS = {
    "gsr_destroy": dict(c=CTX),
    "gsr_reserve": dict(c=CTX, n=8, pairs=64),
    "gsr_preprocess": dict(c=CTX, **FRAME, stream=None),
    "gsr_sort": dict(c=CTX, stream=None),
    "gsr_blend": dict(c=CTX, out=P(4096), stream=None),
    "gsr_render": dict(c=CTX, **FRAME, out=P(4096), stream=None),
    "gsr_render_aux": dict(c=CTX, **FRAME, out=P(4096), aux=aux(), stream=None),
    "gsr_render_contrib": dict(c=CTX, **FRAME, out=contrib(), stream=None),
    "gsr_render_backward": dict(c=CTX, **FRAME, bw=backward(), stream=None),
    "gsr_project_backward": dict(c=CTX, scene=P(0), layout=0, n=8, cam=cam(), W=8, H=8, k=3.0, rec=rec_grads(),
                                 out=scene_grads(), stream=None),
    "gsr_render_backward_scene": dict(c=CTX, **FRAME, gi=P(8192), ga=None, scratch=None, out=scene_grads(),
                                      stream=None),
    "gsr_set_frames_in_flight": dict(c=CTX, frames=4),
    "gsr_frames_in_flight": dict(c=CTX),
    "gsr_render_path": dict(PATH),
    "gsr_render_path_ex": dict(PATH, fev=None, wev=None, flags=0),
    "gsr_render_path_status": dict(PATH, fev=None, wev=None, flags=0, status=None),
    "gsr_sync": dict(c=CTX),
    "gsr_pair_count": dict(c=CTX),
    "gsr_row_item_count": dict(c=CTX),
    "gsr_read_splats": dict(c=CTX, host=P(0), n=0),
    "gsr_depth_passes": dict(c=CTX),
    "gsr_bucket_sizes": dict(c=CTX, sizes=P(0), cap=4),
    "gsr_read_depth_order": dict(c=CTX, host=P(0), n=0),
    "gsr_read_pairs": dict(c=CTX, host=P(0), cap=4),
    "gsr_tile_grid": dict(c=CTX, tx=INT_OUT, ty=INT_OUT),
    "gsr_read_tile_ranges": dict(c=CTX, host=P(0), nt=0),
    "gsr_set_timing": dict(c=CTX, mode=1),
    "gsr_set_timing_stride": dict(c=CTX, mode=2, stride=3),
    "gsr_stage_times": dict(c=CTX, ms=P(0), frames=None),
    "gsr_set_diagnostics": dict(c=CTX, on=1),
    "gsr_set_time": dict(c=CTX, t=0.5),
    "gsr_set_blend_variant": dict(c=CTX, variant=3),
    "gsr_blend_stamps": dict(c=CTX, out=P(0), n=0),
    "gsr_blend_records_loaded": dict(c=CTX),
    "gsr_blend_counters_ex": dict(c=CTX, out=P(0), n=16),
    "gsr_blend_take_map": dict(c=CTX, out=P(0), n=0),
    "gsr_blend_counters": dict(c=CTX, out=P(0)),
    "gsr_get_tuning": dict(c=CTX, knob=0, value=P(0)),
    "gsr_set_tuning": dict(c=CTX, knob=0, value=0),
    "gsr_rank_order_check": dict(ops=I64_OUT, bad=I64_OUT),
    "gsr_math_probe": dict(x=P(0), n=4, out=P(1024)),
    "gsr_exp_probe2": dict(lo=-10.0, hi=0.0, big=-5.0, viol=P(0), packed=P(8), err_all=P(16), err_big=P(24)),
    "gsr_exp_probe": dict(lo=-10.0, hi=0.0, big=-5.0, viol=P(0), err_all=P(16), err_big=P(24)),
    "gsr_alpha_cut_probe": dict(op=P(0), n=4, out=P(1024)),
    "preprocessCUDAGaussians": dict(scene=P(0), out=P(4096), n=8, cam=CAM_VALUE, nty=1, ntx=1, ws=8, hs=8, W=8, H=8,
                                    k=3.0),
}

NULL = "null context"
COUNT_LO = "Gaussian count -1 out of range"
COUNT_HI = "Gaussian count 2147483648 out of range"
SCENE = "null scene"
LAYOUT = "unknown scene layout 7"
CAMERA = "null camera"
SIZE = "image size 0x8 out of range [1, 32768]"
TILING = "bad tiling nx=0 ny=1 ws=8 hs=8"
AUX = "gsr_render_aux: "
CONTRIB = "gsr_render_contrib: "
BACKWARD = "gsr_render_backward: "
PROJECT = "gsr_project_backward: "
FUSED = "gsr_render_backward_scene: "
INFLIGHT = "gsr_set_frames_in_flight: frames must be 1..8"
FLAGS = "gsr_render_path_ex: unknown flags 0x4"
ARRAYS = "gsr_render_path: bad frame arrays"
OUT1 = "gsr_render_path: null output for frame 1"
TIMING = "gsr_set_timing: bad argument"
VARIANT = "gsr_set_blend_variant: variant must be 0 (default) or 3 (timeline stamps)"
COUNTERS = "gsr_blend_counters: diagnostics were off"
COUNTERS_EX = "gsr_blend_counters_ex: diagnostics were off or bad count"
TAKE_MAP = "gsr_blend_take_map: diagnostics were off or bad size"
DROPIN = "bad output buffer or size"

# what every call that plans a frame (preprocess_plan: check_scene_args, then fill_frame) refuses
PLAN = [
    (dict(n=-1), COUNT_LO), (dict(n=BIG), COUNT_HI), (dict(scene=None), SCENE), (dict(layout=7), LAYOUT),
    (dict(layout=-1), "unknown scene layout -1"), (dict(layout=4), "unknown scene layout 4"),
    (dict(n=0, scene=None, layout=7), LAYOUT),         # no Gaussians need no scene
    (dict(cam=None), CAMERA), (dict(W=0), SIZE), (dict(H=0), "image size 8x0 out of range [1, 32768]"),
    (dict(W=32769), "image size 32769x8 out of range [1, 32768]"),
    (dict(H=-3), "image size 8x-3 out of range [1, 32768]"),
    (dict(nx=0), TILING), (dict(ny=-1), "bad tiling nx=1 ny=-1 ws=8 hs=8"),
    (dict(ws=0), "bad tiling nx=1 ny=1 ws=0 hs=8"), (dict(hs=0), "bad tiling nx=1 ny=1 ws=8 hs=0"),
]
PLAN_TWO = [
    (dict(n=-1, layout=7), COUNT_LO), (dict(n=BIG, scene=None), COUNT_HI), (dict(scene=None, layout=7), SCENE),
    (dict(layout=7, cam=None), LAYOUT), (dict(cam=None, W=0), CAMERA), (dict(W=0, nx=0), SIZE),
    (dict(H=0, hs=0), "image size 8x0 out of range [1, 32768]"),
    (dict(nx=0, hs=0), "bad tiling nx=0 ny=1 ws=8 hs=0"),
]
PLANNERS = ("gsr_preprocess", "gsr_render", "gsr_render_aux", "gsr_render_contrib", "gsr_render_backward",
            "gsr_render_backward_scene")


def grads_rows(call, who, arg):
    """check_scene_grads' four texts."""
    return [
        (call, {arg: None}, E, who + "null outputs"),
        (call, {arg: scene_grads(**NO_GRADS)}, E, who + "no output"),
        (call, {arg: scene_grads(), "layout": 1}, E, who + "GSR_LAYOUT_AOS has no gradient planes; upload a scene block"),
        (call, {arg: scene_grads(d_temporal=P(20480))}, E, who + "d_temporal needs a 4D scene block"),
        (call, {arg: scene_grads(d_temporal=P(20480)), "layout": 3}, E, who + "d_temporal needs a 4D scene block"),
        (call, {arg: scene_grads(**NO_GRADS, d_temporal=P(20480)), "layout": 1}, E,
         who + "GSR_LAYOUT_AOS has no gradient planes; upload a scene block"),
    ]


# (call, arguments other than DEFAULTS', what it returns, the text of gsr_last_error; None: the
# call leaves the text alone)
ONE_AT_A_TIME = [
    ("gsr_destroy", dict(c=None), None, None),
    ("gsr_destroy", dict(), None, None),

    ("gsr_reserve", dict(c=None), E, "gsr_reserve: bad argument"),
    ("gsr_reserve", dict(n=-1), E, "gsr_reserve: bad argument"),
    ("gsr_reserve", dict(pairs=-1), E, "gsr_reserve: bad argument"),

    *[(call, dict(c=None), E, NULL) for call in PLANNERS],
    *[(call, over, E, text) for call in PLANNERS for over, text in PLAN],

    ("gsr_sort", dict(c=None), E, NULL),
    ("gsr_sort", dict(), E, "gsr_sort before gsr_preprocess"),
    ("gsr_blend", dict(c=None), E, NULL),
    ("gsr_blend", dict(), E, "gsr_blend before gsr_sort"),

    ("gsr_render_aux", dict(aux=None), E, AUX + "null aux targets"),
    ("gsr_render_aux", dict(aux=aux(nfeat=-1)), E, AUX + "nfeat -1 out of range [0, 8]"),
    ("gsr_render_aux", dict(aux=aux(nfeat=9, d_features=P(20480), d_feat_out=P(24576))), E,
     AUX + "nfeat 9 out of range [0, 8]"),
    ("gsr_render_aux", dict(aux=aux(nfeat=2, d_feat_out=P(24576))), E, AUX + "nfeat 2 needs d_features and d_feat_out"),
    ("gsr_render_aux", dict(aux=aux(nfeat=8, d_features=P(20480))), E, AUX + "nfeat 8 needs d_features and d_feat_out"),
    ("gsr_render_aux", dict(out=None, aux=aux(d_alpha=None)), E, AUX + "no output"),
    # the features' pointers count for nothing while nfeat is 0
    ("gsr_render_aux", dict(out=None, aux=aux(d_alpha=None, d_features=P(20480), d_feat_out=P(24576))), E,
     AUX + "no output"),

    ("gsr_render_contrib", dict(out=None), E, CONTRIB + "null targets"),
    ("gsr_render_contrib", dict(out=contrib(d_count=None)), E, CONTRIB + "no output"),

    ("gsr_render_backward", dict(bw=None), E, BACKWARD + "null targets"),
    ("gsr_render_backward", dict(bw=backward(d_grad_image=None)), E, BACKWARD + "no upstream gradient"),
    ("gsr_render_backward", dict(bw=backward(d_color=None)), E, BACKWARD + "no output"),

    ("gsr_project_backward", dict(c=None), E, NULL),
    ("gsr_project_backward", dict(rec=None), E, PROJECT + "null inputs"),
    ("gsr_project_backward", dict(rec=rec_grads(d_color=None)), E, PROJECT + "no upstream gradient"),
    *grads_rows("gsr_project_backward", PROJECT, "out"),
    ("gsr_project_backward", dict(n=-1), E, COUNT_LO),
    ("gsr_project_backward", dict(n=BIG), E, COUNT_HI),
    ("gsr_project_backward", dict(scene=None), E, SCENE),
    ("gsr_project_backward", dict(layout=7), E, LAYOUT),
    ("gsr_project_backward", dict(cam=None), E, CAMERA),
    ("gsr_project_backward", dict(W=0), E, SIZE),
    ("gsr_project_backward", dict(H=32769), E, "image size 8x32769 out of range [1, 32768]"),
    ("gsr_project_backward", dict(n=0), 0, None),                      # nothing to launch
    ("gsr_project_backward", dict(n=0, scene=None, layout=2, out=scene_grads(d_temporal=P(20480))), 0, None),

    ("gsr_render_backward_scene", dict(gi=None), E, FUSED + "no upstream gradient"),
    *grads_rows("gsr_render_backward_scene", FUSED, "out"),

    ("gsr_set_frames_in_flight", dict(c=None), E, INFLIGHT),
    ("gsr_set_frames_in_flight", dict(frames=0), E, INFLIGHT),
    ("gsr_set_frames_in_flight", dict(frames=9), E, INFLIGHT),
    ("gsr_set_frames_in_flight", dict(frames=-1), E, INFLIGHT),
    ("gsr_set_frames_in_flight", dict(frames=1), 0, None),
    ("gsr_set_frames_in_flight", dict(frames=8), 0, None),
    ("gsr_frames_in_flight", dict(c=None), E, NULL),
    ("gsr_frames_in_flight", dict(), 3, None),

    ("gsr_render_path", dict(c=None), E, NULL),
    ("gsr_render_path", dict(nframes=-1), E, ARRAYS),
    ("gsr_render_path", dict(cams=None), E, ARRAYS),
    ("gsr_render_path", dict(outs=None), E, ARRAYS),
    ("gsr_render_path", dict(outs=A(P(4096), None)), E, OUT1),
    ("gsr_render_path", dict(outs=A(None, None)), E, "gsr_render_path: null output for frame 0"),
    ("gsr_render_path", dict(nframes=0), 0, None),
    ("gsr_render_path", dict(nframes=0, cams=None, outs=None, scene=None, layout=7, W=0), 0, None),
    ("gsr_render_path_ex", dict(c=None), E, NULL),
    ("gsr_render_path_ex", dict(flags=4), E, FLAGS),
    ("gsr_render_path_ex", dict(flags=7), E, "gsr_render_path_ex: unknown flags 0x7"),
    ("gsr_render_path_ex", dict(flags=-1), E, "gsr_render_path_ex: unknown flags 0xffffffff"),
    ("gsr_render_path_ex", dict(nframes=-1), E, ARRAYS),
    ("gsr_render_path_ex", dict(cams=None), E, ARRAYS),
    ("gsr_render_path_ex", dict(outs=None), E, ARRAYS),
    ("gsr_render_path_ex", dict(outs=A(P(4096), None)), E, OUT1),
    ("gsr_render_path_ex", dict(nframes=0, flags=3), 0, None),
    ("gsr_render_path_status", dict(c=None), E, NULL),
    ("gsr_render_path_status", dict(flags=4), E, FLAGS),
    ("gsr_render_path_status", dict(nframes=-2), E, ARRAYS),
    ("gsr_render_path_status", dict(cams=None), E, ARRAYS),
    ("gsr_render_path_status", dict(outs=None), E, ARRAYS),
    ("gsr_render_path_status", dict(outs=A(P(4096), None)), E, OUT1),
    ("gsr_render_path_status", dict(nframes=0), 0, None),
    ("gsr_render_path_status", dict(nframes=0, cams=None, outs=None, flags=1), 0, None),

    ("gsr_sync", dict(c=None), E, NULL),
    ("gsr_sync", dict(), 0, None),                                      # nothing queued, nothing pending

    ("gsr_pair_count", dict(c=None), -1, None),
    ("gsr_pair_count", dict(), -1, None),
    ("gsr_row_item_count", dict(c=None), -1, None),
    ("gsr_row_item_count", dict(), -1, None),
    ("gsr_read_splats", dict(c=None), E, "gsr_read_splats: bad argument"),
    ("gsr_read_splats", dict(host=None), E, "gsr_read_splats: bad argument"),
    ("gsr_read_splats", dict(n=-1), E, "gsr_read_splats: bad argument"),
    ("gsr_read_splats", dict(n=1), E, "gsr_read_splats: bad argument"),        # more than the frame's
    ("gsr_depth_passes", dict(c=None), E, "gsr_depth_passes: no sorted frame"),
    ("gsr_depth_passes", dict(), E, "gsr_depth_passes: no sorted frame"),
    ("gsr_bucket_sizes", dict(c=None), E, "gsr_bucket_sizes: bad argument"),
    ("gsr_bucket_sizes", dict(cap=-1), E, "gsr_bucket_sizes: bad argument"),
    ("gsr_bucket_sizes", dict(sizes=None), E, "gsr_bucket_sizes: bad argument"),
    ("gsr_bucket_sizes", dict(), 0, None),                              # no bucket-sorted frame: no buckets
    ("gsr_bucket_sizes", dict(sizes=None, cap=0), 0, None),
    ("gsr_read_depth_order", dict(c=None), E, "gsr_read_depth_order: bad argument"),
    ("gsr_read_depth_order", dict(host=None), E, "gsr_read_depth_order: bad argument"),
    ("gsr_read_depth_order", dict(n=-1), E, "gsr_read_depth_order: bad argument"),
    ("gsr_read_depth_order", dict(n=1), E, "gsr_read_depth_order: bad argument"),
    ("gsr_read_depth_order", dict(), E, "gsr_read_depth_order: bad argument"),  # no sorted frame
    ("gsr_read_pairs", dict(c=None), E, "gsr_read_pairs: bad argument"),
    ("gsr_read_pairs", dict(host=None), E, "gsr_read_pairs: bad argument"),
    ("gsr_read_pairs", dict(cap=-1), E, "gsr_read_pairs: bad argument"),
    ("gsr_read_pairs", dict(), E, "gsr_read_pairs: bad argument"),              # no sorted frame
    ("gsr_tile_grid", dict(c=None), E, "gsr_tile_grid: bad argument"),
    ("gsr_tile_grid", dict(tx=None), E, "gsr_tile_grid: bad argument"),
    ("gsr_tile_grid", dict(ty=None), E, "gsr_tile_grid: bad argument"),
    ("gsr_tile_grid", dict(), 0, None),                                 # no frame yet: a 0 x 0 grid
    ("gsr_read_tile_ranges", dict(c=None), E, "gsr_read_tile_ranges: bad argument"),
    ("gsr_read_tile_ranges", dict(host=None), E, "gsr_read_tile_ranges: bad argument"),
    ("gsr_read_tile_ranges", dict(nt=-1), E, "gsr_read_tile_ranges: bad argument"),
    ("gsr_read_tile_ranges", dict(nt=1), E, "gsr_read_tile_ranges: bad argument"),
    ("gsr_read_tile_ranges", dict(), E, "gsr_read_tile_ranges: bad argument"),  # no sorted frame

    ("gsr_set_timing", dict(c=None), E, TIMING),
    ("gsr_set_timing", dict(mode=-1), E, TIMING),
    ("gsr_set_timing", dict(mode=3), E, TIMING),
    ("gsr_set_timing", dict(mode=0), 0, None),
    ("gsr_set_timing", dict(), 0, None),
    ("gsr_set_timing", dict(mode=2), 0, None),
    ("gsr_set_timing_stride", dict(c=None), E, TIMING),
    ("gsr_set_timing_stride", dict(mode=-1), E, TIMING),
    ("gsr_set_timing_stride", dict(mode=3), E, TIMING),
    ("gsr_set_timing_stride", dict(stride=0), E, TIMING),
    ("gsr_set_timing_stride", dict(stride=-4), E, TIMING),
    ("gsr_set_timing_stride", dict(), 0, None),
    ("gsr_stage_times", dict(c=None), E, "gsr_stage_times: bad argument"),
    ("gsr_stage_times", dict(ms=None), E, "gsr_stage_times: bad argument"),
    ("gsr_set_diagnostics", dict(c=None), E, NULL),
    ("gsr_set_diagnostics", dict(), 0, None),
    ("gsr_set_diagnostics", dict(on=0), 0, None),
    ("gsr_set_time", dict(c=None), E, NULL),
    ("gsr_set_time", dict(), 0, None),
    ("gsr_set_blend_variant", dict(c=None), E, NULL),
    ("gsr_set_blend_variant", dict(variant=1), E, VARIANT),
    ("gsr_set_blend_variant", dict(variant=2), E, VARIANT),
    ("gsr_set_blend_variant", dict(variant=-1), E, VARIANT),
    ("gsr_set_blend_variant", dict(variant=0), 0, None),
    ("gsr_set_blend_variant", dict(), 0, None),

    ("gsr_blend_stamps", dict(c=None), E, "gsr_blend_stamps: bad argument"),
    ("gsr_blend_stamps", dict(out=None), E, "gsr_blend_stamps: bad argument"),
    ("gsr_blend_stamps", dict(n=-1), E, "gsr_blend_stamps: bad argument"),
    ("gsr_blend_stamps", dict(), E, "gsr_blend_stamps: bad argument"),         # diagnostics were off
    ("gsr_blend_records_loaded", dict(c=None), -1, COUNTERS),
    ("gsr_blend_records_loaded", dict(), -1, COUNTERS),
    ("gsr_blend_counters_ex", dict(c=None), E, COUNTERS_EX),
    ("gsr_blend_counters_ex", dict(out=None), E, COUNTERS_EX),
    ("gsr_blend_counters_ex", dict(n=-1), E, COUNTERS_EX),
    ("gsr_blend_counters_ex", dict(n=17), E, COUNTERS_EX),
    ("gsr_blend_counters_ex", dict(), E, COUNTERS_EX),
    ("gsr_blend_take_map", dict(c=None), E, TAKE_MAP),
    ("gsr_blend_take_map", dict(out=None), E, TAKE_MAP),
    ("gsr_blend_take_map", dict(n=64), E, TAKE_MAP),
    ("gsr_blend_take_map", dict(), E, TAKE_MAP),
    ("gsr_blend_counters", dict(c=None), E, COUNTERS),
    ("gsr_blend_counters", dict(out=None), E, COUNTERS),
    ("gsr_blend_counters", dict(), E, COUNTERS),

    ("gsr_get_tuning", dict(c=None), E, "gsr_get_tuning: null argument"),
    ("gsr_get_tuning", dict(value=None), E, "gsr_get_tuning: null argument"),
    ("gsr_set_tuning", dict(c=None), E, NULL),
    ("gsr_rank_order_check", dict(ops=None), E, "gsr_rank_order_check: null argument"),
    ("gsr_rank_order_check", dict(bad=None), E, "gsr_rank_order_check: null argument"),

    ("gsr_math_probe", dict(x=None), E, "gsr_math_probe: bad argument"),
    ("gsr_math_probe", dict(out=None), E, "gsr_math_probe: bad argument"),
    ("gsr_math_probe", dict(n=0), E, "gsr_math_probe: bad argument"),
    ("gsr_math_probe", dict(n=-1), E, "gsr_math_probe: bad argument"),
    ("gsr_exp_probe2", dict(viol=None), E, "gsr_exp_probe: bad argument"),
    ("gsr_exp_probe2", dict(packed=None), E, "gsr_exp_probe: bad argument"),
    ("gsr_exp_probe2", dict(err_all=None), E, "gsr_exp_probe: bad argument"),
    ("gsr_exp_probe2", dict(err_big=None), E, "gsr_exp_probe: bad argument"),
    ("gsr_exp_probe2", dict(lo=0.0), E, "gsr_exp_probe: bad argument"),
    ("gsr_exp_probe2", dict(lo=1.0), E, "gsr_exp_probe: bad argument"),
    ("gsr_exp_probe2", dict(hi=float("nan")), E, "gsr_exp_probe: bad argument"),
    ("gsr_exp_probe", dict(viol=None), E, "gsr_exp_probe: bad argument"),
    ("gsr_exp_probe", dict(err_all=None), E, "gsr_exp_probe: bad argument"),
    ("gsr_exp_probe", dict(err_big=None), E, "gsr_exp_probe: bad argument"),
    ("gsr_exp_probe", dict(lo=0.0), E, "gsr_exp_probe: bad argument"),
    ("gsr_alpha_cut_probe", dict(op=None), E, "gsr_alpha_cut_probe: bad argument"),
    ("gsr_alpha_cut_probe", dict(out=None), E, "gsr_alpha_cut_probe: bad argument"),
    ("gsr_alpha_cut_probe", dict(n=0), E, "gsr_alpha_cut_probe: bad argument"),
    ("gsr_alpha_cut_probe", dict(n=-1), E, "gsr_alpha_cut_probe: bad argument"),

    # the drop-in frame call returns nothing: the text (which it also prints) is all there is
    ("preprocessCUDAGaussians", dict(out=None), None, DROPIN),
    ("preprocessCUDAGaussians", dict(W=0), None, DROPIN),
    ("preprocessCUDAGaussians", dict(H=-1), None, DROPIN),
]

# two bad arguments at once: the check that comes first reports
TWO_AT_ONCE = [
    ("gsr_reserve", dict(c=None, n=-1), E, "gsr_reserve: bad argument"),
    *[(call, dict(over, c=None), E, NULL) for call in PLANNERS for over, _ in PLAN_TWO[:1]],
    *[(call, over, E, text) for call in PLANNERS for over, text in PLAN_TWO],
    ("gsr_blend", dict(out=None), E, "gsr_blend before gsr_sort"),
    ("gsr_blend", dict(c=None, out=None), E, NULL),
    ("gsr_render", dict(out=None, layout=7), E, LAYOUT),               # the output is the blend's to refuse
    ("gsr_render_aux", dict(c=None, aux=None), E, NULL),
    ("gsr_render_aux", dict(aux=None, layout=7), E, AUX + "null aux targets"),
    ("gsr_render_aux", dict(aux=aux(nfeat=9)), E, AUX + "nfeat 9 out of range [0, 8]"),
    ("gsr_render_aux", dict(out=None, aux=aux(d_alpha=None, nfeat=3)), E, AUX + "nfeat 3 needs d_features and d_feat_out"),
    ("gsr_render_aux", dict(out=None, aux=aux(d_alpha=None), n=-1), E, AUX + "no output"),
    ("gsr_render_contrib", dict(c=None, out=None), E, NULL),
    ("gsr_render_contrib", dict(out=None, n=-1), E, CONTRIB + "null targets"),
    ("gsr_render_contrib", dict(out=contrib(d_count=None), cam=None), E, CONTRIB + "no output"),
    ("gsr_render_backward", dict(c=None, bw=None), E, NULL),
    ("gsr_render_backward", dict(bw=None, W=0), E, BACKWARD + "null targets"),
    ("gsr_render_backward", dict(bw=backward(d_grad_image=None, d_color=None)), E, BACKWARD + "no upstream gradient"),
    ("gsr_render_backward", dict(bw=backward(d_color=None), scene=None), E, BACKWARD + "no output"),
    ("gsr_project_backward", dict(c=None, rec=None), E, NULL),
    ("gsr_project_backward", dict(rec=None, out=None), E, PROJECT + "null inputs"),
    ("gsr_project_backward", dict(rec=rec_grads(d_color=None), out=None), E, PROJECT + "no upstream gradient"),
    ("gsr_project_backward", dict(out=None, n=-1), E, PROJECT + "null outputs"),
    ("gsr_project_backward", dict(out=scene_grads(**NO_GRADS), layout=1), E, PROJECT + "no output"),
    ("gsr_project_backward", dict(layout=1, n=-1), E, PROJECT + "GSR_LAYOUT_AOS has no gradient planes; upload a scene block"),
    ("gsr_project_backward", dict(out=scene_grads(d_temporal=P(20480)), layout=7), E,
     PROJECT + "d_temporal needs a 4D scene block"),
    ("gsr_project_backward", dict(n=-1, cam=None), E, COUNT_LO),
    ("gsr_project_backward", dict(layout=7, W=0), E, LAYOUT),
    ("gsr_project_backward", dict(cam=None, H=0), E, CAMERA),
    ("gsr_project_backward", dict(n=0, W=0), E, SIZE),
    ("gsr_render_backward_scene", dict(c=None, gi=None), E, NULL),
    ("gsr_render_backward_scene", dict(gi=None, out=None), E, FUSED + "no upstream gradient"),
    ("gsr_render_backward_scene", dict(out=None, n=-1), E, FUSED + "null outputs"),
    ("gsr_render_backward_scene", dict(out=scene_grads(d_temporal=P(20480)), layout=7), E,
     FUSED + "d_temporal needs a 4D scene block"),
    ("gsr_render_backward_scene", dict(layout=1, nx=0), E, FUSED + "GSR_LAYOUT_AOS has no gradient planes; upload a scene block"),
    ("gsr_set_frames_in_flight", dict(c=None, frames=0), E, INFLIGHT),
    ("gsr_render_path", dict(c=None, nframes=-1), E, NULL),
    ("gsr_render_path", dict(nframes=-1, outs=A(P(4096), None)), E, ARRAYS),
    ("gsr_render_path", dict(cams=None, outs=A(P(4096), None)), E, ARRAYS),
    ("gsr_render_path", dict(outs=A(P(4096), None), layout=7), E, OUT1),
    ("gsr_render_path_ex", dict(c=None, flags=4), E, NULL),
    ("gsr_render_path_ex", dict(flags=4, nframes=-1), E, FLAGS),
    ("gsr_render_path_ex", dict(flags=4, nframes=0), E, FLAGS),
    ("gsr_render_path_ex", dict(nframes=-1, outs=None), E, ARRAYS),
    ("gsr_render_path_ex", dict(outs=A(P(4096), None), n=-1), E, OUT1),
    ("gsr_render_path_status", dict(c=None, flags=4), E, NULL),
    ("gsr_render_path_status", dict(flags=4, cams=None), E, FLAGS),
    ("gsr_render_path_status", dict(cams=None, outs=A(None, None)), E, ARRAYS),
    ("gsr_render_path_status", dict(outs=A(None, None), W=0), E, "gsr_render_path: null output for frame 0"),
    ("gsr_read_splats", dict(c=None, host=None), E, "gsr_read_splats: bad argument"),
    ("gsr_bucket_sizes", dict(c=None, cap=-1), E, "gsr_bucket_sizes: bad argument"),
    ("gsr_tile_grid", dict(tx=None, ty=None), E, "gsr_tile_grid: bad argument"),
    ("gsr_set_timing", dict(c=None, mode=3), E, TIMING),
    ("gsr_set_timing_stride", dict(mode=3, stride=0), E, TIMING),
    ("gsr_stage_times", dict(c=None, ms=None), E, "gsr_stage_times: bad argument"),
    ("gsr_set_blend_variant", dict(c=None, variant=1), E, NULL),
    ("gsr_blend_counters_ex", dict(out=None, n=17), E, COUNTERS_EX),
    ("gsr_get_tuning", dict(c=None, value=None), E, "gsr_get_tuning: null argument"),
    ("gsr_get_tuning", dict(value=None, knob=99), E, "gsr_get_tuning: null argument"),
    ("gsr_set_tuning", dict(c=None, knob=99), E, NULL),
    ("gsr_rank_order_check", dict(ops=None, bad=None), E, "gsr_rank_order_check: null argument"),
    ("gsr_math_probe", dict(x=None, n=0), E, "gsr_math_probe: bad argument"),
    ("gsr_exp_probe2", dict(viol=None, lo=1.0), E, "gsr_exp_probe: bad argument"),
    ("gsr_alpha_cut_probe", dict(op=None, n=0), E, "gsr_alpha_cut_probe: bad argument"),
    ("preprocessCUDAGaussians", dict(out=None, W=0), None, DROPIN),
]

TABLE = ONE_AT_A_TIME + TWO_AT_ONCE
# calls no row of which is refused / whose every refusal is one text for any bad argument
NO_ARGUMENT_ERROR = {"gsr_destroy", "gsr_pair_count", "gsr_row_item_count"}
ONE_TEXT_ONE_ARGUMENT = {"gsr_sort", "gsr_frames_in_flight", "gsr_sync", "gsr_depth_passes", "gsr_set_diagnostics",
                         "gsr_set_time", "gsr_blend_records_loaded", "gsr_read_depth_order", "gsr_read_pairs",
                         "gsr_read_tile_ranges", "gsr_blend_stamps", "gsr_blend_take_map", "gsr_blend_counters",
                         "gsr_exp_probe"}


def test_the_table_covers_every_entry_point():
    calls = {row[0] for row in TABLE}
    assert calls == set(DEFAULTS)
    refused = {row[0] for row in TABLE if row[3] is not None}
    assert refused == set(DEFAULTS) - NO_ARGUMENT_ERROR
    assert {row[0] for row in TWO_AT_ONCE} == set(DEFAULTS) - NO_ARGUMENT_ERROR - ONE_TEXT_ONE_ARGUMENT
    for call, over, _, _ in TABLE:
        assert set(over) <= set(DEFAULTS[call]), (call, over)


@pytest.fixture(scope="module")
def host(gsr):
    """The host buffer the "device" pointers point into."""
    buf = (ctypes.c_uint64 * 4096)()
    return buf, ctypes.addressof(buf)


KNOWN = "gsr_scene_bytes: bad argument"   # a text put there before a row that must leave it alone


@pytest.mark.parametrize("row", range(len(TABLE)), ids=lambda i: f"{TABLE[i][0]}-{i}")
def test_row(gsr, host, row, capfd):
    from gaussianrenderer_amd import _native
    call, over, want, text = TABLE[row]
    buf, base = host
    L = gsr.lib()
    keep = []       # what the call's pointers point to
    contexts = []

    def resolve(v):
        if isinstance(v, P):
            return base + v.off
        if isinstance(v, S):
            st = getattr(_native, v.ctype)(**{k: resolve(f) for k, f in v.fields.items()})
            keep.append(st)
            return ctypes.byref(st)
        if isinstance(v, A):
            arr = (ctypes.c_void_p * len(v.items))(*[resolve(i) for i in v.items])
            keep.append(arr)
            return ctypes.cast(arr, ctypes.c_void_p)
        if v is CTX:
            contexts.append(L.gsr_create())
            assert contexts[-1]
            return contexts[-1]
        if v is CAMS:
            keep.append((_native.Camera * 2)())
            return keep[-1]
        if v is CAM_VALUE:
            return _native.Camera()
        if v is INT_OUT or v is I64_OUT:
            keep.append((ctypes.c_int if v is INT_OUT else ctypes.c_int64)(-7))
            return ctypes.byref(keep[-1])
        return v

    args = dict(DEFAULTS[call])
    args.update(over)
    if text is None:   # the call leaves the text alone: put a known one there
        assert L.gsr_scene_bytes(0, 0) == E and L.gsr_last_error() == KNOWN.encode()
    fn = getattr(L, call)
    resolved = [resolve(v) for v in args.values()]
    # a buffer address for a typed pointer parameter (gsr_stage_times' double*)
    resolved = [ctypes.cast(ctypes.c_void_p(v), t) if isinstance(v, int) and hasattr(t, "contents") else v
                for v, t in zip(resolved, fn.argtypes)]
    got = fn(*resolved)
    if call == "gsr_destroy":
        contexts.clear()
    assert got == want, (call, over, L.gsr_last_error())
    assert L.gsr_last_error().decode() == (KNOWN if text is None else text), (call, over)
    if call == "preprocessCUDAGaussians":   # it also prints what it refused
        assert f"preprocessCUDAGaussians: argument: {text}" in capfd.readouterr().err
    # outputs: an error leaves them alone; gsr_tile_grid before any frame reads a 0 x 0 grid
    for out in keep:
        if isinstance(out, (ctypes.c_int, ctypes.c_int64)):
            assert out.value == (0 if text is None else -7), (call, over)
    assert not any(buf), (call, over)
    for c in contexts:
        L.gsr_destroy(c)


def test_frames_in_flight_reads_back(gsr):
    """Every accepted count reads back; a refused one leaves the earlier count."""
    L = gsr.lib()
    c = L.gsr_create()
    try:
        assert L.gsr_frames_in_flight(c) == 3
        for f in range(1, 9):
            assert L.gsr_set_frames_in_flight(c, f) == 0 and L.gsr_frames_in_flight(c) == f
        for f in (0, 9, -1):
            assert L.gsr_set_frames_in_flight(c, f) == E and L.gsr_frames_in_flight(c) == 8
    finally:
        L.gsr_destroy(c)
