"""ctypes binding of libgsr.so (the C ABI declared in include/gsr.h).

The shared library is built in-tree by ``make`` (``__graft_entry__.build()``)
into ``gaussianrenderer_amd/lib/libgsr.so``.  There is no Python or CPU
fallback for anything that renders: if the library is missing, importing this
module raises.

Import torch BEFORE this module in processes that use both: torch ships its
own ``libamdhip64.so`` (SONAME ``libamdhip64.so.7``) and the dynamic loader
then binds libgsr to that same HIP runtime instead of loading a second one.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int64, c_uint32, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
# GSR_LIBRARY: another build of the same library (tools/ab_libs.sh A/B runs of two builds
# on one box); the product default is the in-tree build.
LIB_PATH = os.environ.get("GSR_LIBRARY") or os.path.join(_HERE, "lib", "libgsr.so")

GSR_OK = 0
GSR_E_ARG = -1
GSR_E_HIP = -2
GSR_E_IO = -3
GSR_E_FORMAT = -4
GSR_E_OVERFLOW = -5
GSR_PATH_NO_JOIN = 1   # gsr_render_path_ex flags (include/gsr.h)
GSR_PATH_NO_FORK = 2
GSR_E_DISPLAY = -6
GSR_FRAME_PAIR_OVERFLOW = 1   # gsr_render_path_status validity bits (include/gsr.h)
GSR_FRAME_DEPTH_PASSES = 2
GSR_FRAME_SPEC_MISS = 4

LAYOUT_SCENE_BLOCK = 0
LAYOUT_AOS = 1
LAYOUT_SCENE_BLOCK_4D = 2
LAYOUT_SCENE_BLOCK_SH3 = 3
PLY_TYPED = 1
PLY_SH3 = 2

STAGES = ("preprocess", "depth_sort", "emit", "tile_sort", "ranges", "blend", "resume")
NUM_STAGES = len(STAGES)
TILE_PX = 16
SPLAT_RECORD_BYTES = 64
SCENE_NARRAYS = 38
SCENE4D_NARRAYS = 49
SCENE_SH3_NARRAYS = 59
SCENE_HEADER_BYTES = 256


class Camera(ctypes.Structure):
    """Layout-identical to the reference ``Camera`` (scene/camera.hpp:2-41), 484 B."""

    _fields_ = [
        ("position", c_float * 3),
        ("lookAt", c_float * 3),
        ("w_up", c_float * 3),
        ("fovY", c_float),
        ("aspectRatio", c_float),
        ("nearClip", c_float),
        ("farClip", c_float),
        ("forward_vec", c_float * 3),
        ("right_vec", c_float * 3),
        ("up_vec", c_float * 3),
        ("P_matrix", c_float * 16),
        ("V_matrix", c_float * 16),
        ("M_matrix", c_float * 16),
        ("f_axis", c_float * 3),
        ("r_axis", c_float * 3),
        ("u_axis", c_float * 3),
        ("r_cam", c_float * 9),
        ("r_cam_T", c_float * 9),
        ("plane_normals", c_float * 24),
    ]


assert ctypes.sizeof(Camera) == 484


class Lwg(ctypes.Structure):
    """``lightWeightGaussian`` (utils/gaussians.hpp:32-35), 16 B."""

    _fields_ = [("radix_id", c_uint64), ("gaussian_id", c_uint32)]


assert ctypes.sizeof(Lwg) == 16

AUX_MAX_FEATURES = 8   # GSR_AUX_MAX_FEATURES


class AuxTargets(ctypes.Structure):
    """``gsr_aux_targets`` (include/gsr.h): the extra outputs of gsr_render_aux."""

    _fields_ = [
        ("d_alpha", c_void_p),
        ("d_depth", c_void_p),
        ("d_features", c_void_p),
        ("nfeat", c_int),
        ("d_feat_out", c_void_p),
    ]


CONTRIB_WEIGHT_ONE = 1 << 24   # GSR_CONTRIB_WEIGHT_ONE


class ContribTargets(ctypes.Structure):
    """``gsr_contrib_targets`` (include/gsr.h): the outputs of gsr_render_contrib."""

    _fields_ = [
        ("d_count", c_void_p),
        ("d_weight", c_void_p),
        ("d_max", c_void_p),
        ("d_id", c_void_p),
    ]


class BackwardTargets(ctypes.Structure):
    """``gsr_backward_targets`` (include/gsr.h): the inputs and outputs of gsr_render_backward."""

    _fields_ = [
        ("d_grad_image", c_void_p),
        ("d_grad_alpha", c_void_p),
        ("d_color", c_void_p),
        ("d_opacity", c_void_p),
        ("d_conic", c_void_p),
        ("d_center", c_void_p),
    ]


class RecordGrads(ctypes.Structure):
    """``gsr_record_grads`` (include/gsr.h): the inputs of gsr_project_backward."""

    _fields_ = [
        ("d_color", c_void_p),
        ("d_opacity", c_void_p),
        ("d_conic", c_void_p),
        ("d_center", c_void_p),
    ]


class AuxUpstream(ctypes.Structure):
    """``gsr_aux_upstream`` (include/gsr.h): the upstream gradients of gsr_render_backward_aux and
    the per-Gaussian feature values its feature channels composite."""

    _fields_ = [
        ("d_grad_image", c_void_p),
        ("d_grad_alpha", c_void_p),
        ("d_grad_depth", c_void_p),
        ("d_grad_feat", c_void_p),
        ("d_features", c_void_p),
        ("nfeat", c_int),
    ]


class RecordGradsAuxOut(ctypes.Structure):
    """``gsr_record_grads_aux_out`` (include/gsr.h): the outputs of gsr_render_backward_aux."""

    _fields_ = [
        ("d_color", c_void_p),
        ("d_opacity", c_void_p),
        ("d_conic", c_void_p),
        ("d_center", c_void_p),
        ("d_z", c_void_p),
        ("d_feat", c_void_p),
    ]


class RecordGradsAux(ctypes.Structure):
    """``gsr_record_grads_aux`` (include/gsr.h): the inputs of gsr_project_backward_aux."""

    _fields_ = [
        ("d_color", c_void_p),
        ("d_opacity", c_void_p),
        ("d_conic", c_void_p),
        ("d_center", c_void_p),
        ("d_z", c_void_p),
    ]


class SceneGrads(ctypes.Structure):
    """``gsr_scene_grads`` (include/gsr.h): the outputs of gsr_project_backward and
    gsr_render_backward_scene."""

    _fields_ = [
        ("d_position", c_void_p),
        ("d_opacity", c_void_p),
        ("d_scale", c_void_p),
        ("d_rot", c_void_p),
        ("d_sh", c_void_p),
        ("d_temporal", c_void_p),
    ]


ADAM_SKIP_ZERO = 1    # gsr_adam_config flags (include/gsr.h)
ADAM_ZERO_GRADS = 2
ADAM_OPACITY_MIN = 1e-6        # GSR_ADAM_OPACITY_MIN / MAX, as float32 values
ADAM_OPACITY_MAX = 0.999999


class AdamConfig(ctypes.Structure):
    """``gsr_adam_config`` (include/gsr.h): learning rates per group, betas, eps, step, flags."""

    _fields_ = [
        ("lr_position", c_float), ("lr_opacity", c_float), ("lr_scale", c_float), ("lr_rot", c_float),
        ("lr_sh_dc", c_float), ("lr_sh_rest", c_float),
        ("lr_tcenter", c_float), ("lr_tscale", c_float), ("lr_motion", c_float),
        ("beta1", c_float), ("beta2", c_float), ("eps", c_float),
        ("step", c_int64),
        ("flags", c_int),
    ]


class DensifyConfig(ctypes.Structure):
    """``gsr_densify_config`` (include/gsr.h): the thresholds of gsr_scene_densify, the split
    children's shrink factor, the sampler's seed, flags."""

    _fields_ = [
        ("grad_threshold", c_float), ("scale_split", c_float), ("min_opacity", c_float),
        ("prune_scale_max", c_float), ("split_shrink", c_float),
        ("seed", c_uint64),
        ("flags", c_int),
    ]


class DensifyReport(ctypes.Structure):
    """``gsr_densify_report`` (include/gsr.h): the outputs and the sources by fate."""

    _fields_ = [("n_out", c_int64), ("kept", c_int64), ("cloned", c_int64), ("split", c_int64), ("pruned", c_int64)]


DENSIFY_CHUNK = 1024   # kDensifyChunk (gsr_internal.h): sources per workgroup of the expansion


class InitConfig(ctypes.Structure):
    """``gsr_init_config`` (include/gsr.h): what gsr_scene_from_points fills a new block with."""

    _fields_ = [
        ("opacity", c_float), ("min_dist2", c_float), ("scale_mul", c_float), ("scale_max", c_float),
        ("t_center", c_float), ("t_scale", c_float),
        ("flags", c_int),
    ]


# the k-NN structure's constants (gsr_internal.h): points per leaf, boxes per coarser box,
# points per workgroup of the bounds kernel, items per workgroup of a sort pass
KNN_LEAF = 64
KNN_FAN = 64
KNN_BOUNDS_CHUNK = 2048
KNN_SORT_TILE = 4096
SH_C0 = 0.28209479177387814   # the preprocess's constant: colour = 0.5 + SH_C0 * dc

LOSS_NVALUES = 4   # GSR_LOSS_NVALUES: d_loss = {L, mean |x-y|, mean (x-y)^2, mean SSIM}


class LossConfig(ctypes.Structure):
    """``gsr_loss_config`` (include/gsr.h): the three weights, the gradient's scale, flags."""

    _fields_ = [("w_l1", c_float), ("w_l2", c_float), ("w_dssim", c_float), ("grad_scale", c_float), ("flags", c_int)]


# (name, restype, argtypes) for every symbol of include/gsr.h and include/gsr_gl.h.
SIGNATURES = [
    ("preprocessCUDAGaussians", None,
     [c_void_p, POINTER(c_float), c_int, Camera, c_int, c_int, c_int, c_int, c_int, c_int, c_float]),
    ("gsr_load_ply_device", c_void_p, [c_char_p, POINTER(c_int)]),
    ("gsr_load_ply_device_ex", c_void_p, [c_char_p, POINTER(c_int), c_int, POINTER(c_int)]),
    ("oneSweep3DGaussianSort", None, [POINTER(Lwg), c_int, c_int, POINTER(c_float)]),
    ("oneSweepSort", None, [POINTER(c_int), POINTER(c_int), c_int, c_int, POINTER(c_float)]),
    # include/gsr_gl.h: display interop (SSBO written in place, no host round trip)
    ("preprocessCUDAGaussiansGL", None,
     [c_void_p, ctypes.c_uint, c_int, Camera, c_int, c_int, c_int, c_int, c_int, c_int, c_float]),
    ("gsr_display_register_gl", c_int, [ctypes.c_uint, POINTER(c_void_p)]),
    ("gsr_display_wrap_device", c_int, [c_void_p, ctypes.c_size_t, POINTER(c_void_p)]),
    ("gsr_display_free", c_int, [c_void_p]),
    ("gsr_display_gl_current", c_int, []),
    ("gsr_render_display", c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int64, POINTER(Camera), c_int, c_int,
                                   c_int, c_int, c_int, c_int, c_float, c_void_p]),
    ("gsr_create", c_void_p, []),
    ("gsr_destroy", None, [c_void_p]),
    ("gsr_reserve", c_int, [c_void_p, c_int64, c_int64]),
    ("gsr_render", c_int, [c_void_p, c_void_p, c_int, c_int64, POINTER(Camera), c_int, c_int, c_int, c_int,
                           c_int, c_int, c_float, c_void_p, c_void_p]),
    ("gsr_render_aux", c_int, [c_void_p, c_void_p, c_int, c_int64, POINTER(Camera), c_int, c_int, c_int, c_int,
                               c_int, c_int, c_float, c_void_p, POINTER(AuxTargets), c_void_p]),
    ("gsr_render_contrib", c_int, [c_void_p, c_void_p, c_int, c_int64, POINTER(Camera), c_int, c_int, c_int, c_int,
                                   c_int, c_int, c_float, POINTER(ContribTargets), c_void_p]),
    ("gsr_render_backward", c_int, [c_void_p, c_void_p, c_int, c_int64, POINTER(Camera), c_int, c_int, c_int, c_int,
                                    c_int, c_int, c_float, POINTER(BackwardTargets), c_void_p]),
    ("gsr_project_backward", c_int, [c_void_p, c_void_p, c_int, c_int64, POINTER(Camera), c_int, c_int, c_float,
                                     POINTER(RecordGrads), POINTER(SceneGrads), c_void_p]),
    ("gsr_render_backward_scene", c_int, [c_void_p, c_void_p, c_int, c_int64, POINTER(Camera), c_int, c_int, c_int,
                                          c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p,
                                          POINTER(SceneGrads), c_void_p]),
    ("gsr_render_backward_aux", c_int, [c_void_p, c_void_p, c_int, c_int64, POINTER(Camera), c_int, c_int, c_int,
                                        c_int, c_int, c_int, c_float, POINTER(AuxUpstream),
                                        POINTER(RecordGradsAuxOut), c_void_p]),
    ("gsr_project_backward_aux", c_int, [c_void_p, c_void_p, c_int, c_int64, POINTER(Camera), c_int, c_int, c_float,
                                         POINTER(RecordGradsAux), POINTER(SceneGrads), c_void_p]),
    ("gsr_render_backward_scene_aux", c_int, [c_void_p, c_void_p, c_int, c_int64, POINTER(Camera), c_int, c_int,
                                              c_int, c_int, c_int, c_int, c_float, POINTER(AuxUpstream), c_void_p,
                                              c_void_p, POINTER(SceneGrads), c_void_p]),
    ("gsr_render_path", c_int, [c_void_p, c_void_p, c_int, c_int64, POINTER(Camera), c_void_p, c_int, c_int,
                                c_int, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p]),
    ("gsr_render_path_ex", c_int, [c_void_p, c_void_p, c_int, c_int64, POINTER(Camera), c_void_p, c_int, c_int,
                                   c_int, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_int]),
    ("gsr_render_path_status", c_int, [c_void_p, c_void_p, c_int, c_int64, POINTER(Camera), c_void_p, c_int,
                                       c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_int, c_void_p]),
    ("gsr_set_frames_in_flight", c_int, [c_void_p, c_int]),
    ("gsr_frames_in_flight", c_int, [c_void_p]),
    ("gsr_preprocess", c_int, [c_void_p, c_void_p, c_int, c_int64, POINTER(Camera), c_int, c_int, c_int, c_int,
                               c_int, c_int, c_float, c_void_p]),
    ("gsr_sort", c_int, [c_void_p, c_void_p]),
    ("gsr_blend", c_int, [c_void_p, c_void_p, c_void_p]),
    ("gsr_sync", c_int, [c_void_p]),
    ("gsr_pair_count", c_int64, [c_void_p]),
    ("gsr_row_item_count", c_int64, [c_void_p]),
    ("gsr_read_splats", c_int, [c_void_p, c_void_p, c_int64]),
    ("gsr_read_depth_order", c_int, [c_void_p, c_void_p, c_int64]),
    ("gsr_read_pairs", c_int64, [c_void_p, c_void_p, c_int64]),
    ("gsr_tile_grid", c_int, [c_void_p, POINTER(c_int), POINTER(c_int)]),
    ("gsr_read_tile_ranges", c_int, [c_void_p, c_void_p, c_int64]),
    ("gsr_set_timing", c_int, [c_void_p, c_int]),
    ("gsr_stage_times", c_int, [c_void_p, POINTER(c_double), POINTER(c_int64)]),
    ("gsr_set_diagnostics", c_int, [c_void_p, c_int]),
    ("gsr_blend_records_loaded", c_int64, [c_void_p]),
    ("gsr_blend_counters", c_int, [c_void_p, c_void_p]),
    ("gsr_set_blend_variant", c_int, [c_void_p, c_int]),
    ("gsr_blend_stamps", c_int, [c_void_p, c_void_p, c_int64]),
    ("gsr_blend_counters_ex", c_int, [c_void_p, c_void_p, c_int]),
    ("gsr_blend_take_map", c_int, [c_void_p, c_void_p, c_int64]),
    ("gsr_set_tuning", c_int, [c_void_p, c_int, c_int]),
    ("gsr_get_tuning", c_int, [c_void_p, c_int, c_void_p]),
    ("gsr_set_timing_stride", c_int, [c_void_p, c_int, c_int]),
    ("gsr_depth_passes", c_int, [c_void_p]),
    ("gsr_bucket_sizes", c_int, [c_void_p, c_void_p, c_int]),
    ("gsr_scene_upload", c_void_p, [c_void_p, c_int64]),
    ("gsr_scene_upload_ex", c_void_p, [c_void_p, c_int, c_int64]),
    ("gsr_set_time", c_int, [c_void_p, c_float]),
    ("gsr_scene_free", None, [c_void_p]),
    ("gsr_scene_download", c_int, [c_void_p, c_void_p, c_int64]),
    ("gsr_scene_bytes", c_int64, [c_int, c_int64]),
    ("gsr_scene_copy", c_int, [c_void_p, c_void_p, c_int, c_int64, c_void_p]),
    # scene editing (include/gsr.h)
    ("gsr_mask_indices", c_int, [c_void_p, c_int64, c_void_p, POINTER(c_int64), c_void_p]),
    ("gsr_gather_planes", c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int, c_int, c_int64, c_void_p, c_int64,
                                  c_void_p, c_void_p]),
    ("gsr_scene_gather", c_void_p, [c_void_p, c_int, c_int64, c_void_p, c_int64, c_void_p, c_void_p]),
    ("gsr_scene_select", c_void_p, [c_void_p, c_int, c_int64, c_void_p, POINTER(c_int64), c_void_p, c_void_p]),
    # scene optimisation (include/gsr.h)
    ("gsr_scene_adam_step", c_int, [c_void_p, c_int, c_int64, POINTER(SceneGrads), POINTER(SceneGrads),
                                    POINTER(SceneGrads), POINTER(AdamConfig), c_void_p, c_void_p]),
    # scene densification (include/gsr.h)
    ("gsr_densify_accumulate", c_int, [c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    ("gsr_scene_densify", c_void_p, [c_void_p, c_int, c_int64, c_void_p, c_void_p, POINTER(DensifyConfig), c_void_p,
                                     c_void_p, POINTER(DensifyReport), c_void_p]),
    ("gsr_densify_normals", None, [c_uint64, c_uint32, c_uint32, c_void_p]),
    ("gsr_logf_probe", c_int, [c_void_p, c_int, c_void_p]),
    ("gsr_densify_gather_planes", c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int, c_int64, c_void_p, c_void_p,
                                          c_int64, c_void_p, c_void_p]),
    ("gsr_scene_reset_opacity", c_int, [c_void_p, c_int, c_int64, c_float, c_void_p, c_void_p, c_void_p]),
    # scene initialisation (include/gsr.h)
    ("gsr_points_knn_scratch_bytes", c_int64, [c_int64]),
    ("gsr_points_knn_dist2", c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
                                     ctypes.c_size_t, c_void_p]),
    ("gsr_scene_from_points", c_void_p, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_int64, c_int,
                                         POINTER(InitConfig), c_void_p, c_void_p, c_void_p]),
    # image loss (include/gsr.h)
    ("gsr_image_loss_scratch_bytes", c_int64, [c_int, c_int, c_int]),
    ("gsr_image_loss", c_int, [c_void_p, c_void_p, c_int, c_int, POINTER(LossConfig), c_void_p, c_void_p, c_void_p,
                               c_int64, c_void_p]),
    # scene export (include/gsr.h)
    ("gsr_ply_row_floats", c_int64, [c_int]),
    ("gsr_scene_pack_rows", c_int, [c_void_p, c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p]),
    ("gsr_scene_save_ply", c_int, [c_void_p, c_int, c_int64, c_char_p, c_int64, c_void_p]),
    ("gsr_ply_write_host", c_int, [c_char_p, c_void_p, c_int, c_int64]),
    ("gsr_raw_probe", c_int, [c_void_p, c_int, c_int, c_void_p]),
    ("gsr_ply_read_host", c_int, [c_char_p, c_void_p, c_int64, POINTER(c_int64)]),
    ("gsr_ply_read_host_ex", c_int, [c_char_p, c_void_p, c_int, c_int64, POINTER(c_int64), c_int, POINTER(c_int)]),
    ("gsr_synth_write_ply", c_int, [c_char_p, c_int64, c_uint64]),
    ("gsr_synth_write_ply4d", c_int, [c_char_p, c_int64, c_uint64]),
    ("gsr_camera_default", None, [POINTER(Camera)]),
    ("gsr_camera_update", None, [POINTER(Camera)]),
    ("gsr_camera_update_frustum", None, [POINTER(Camera)]),
    ("gsr_camera_zoom", None, [POINTER(Camera), c_float]),
    ("gsr_camera_orbit", None, [POINTER(Camera), c_float, c_float]),
    ("gsr_camera_intrinsics", None, [POINTER(Camera), POINTER(c_float), POINTER(c_float)]),
    ("gsr_last_error", c_char_p, []),
    ("gsr_version", c_char_p, []),
    ("gsr_device_available", c_int, []),
    ("gsr_math_probe", c_int, [c_void_p, c_int, c_void_p]),
    ("gsr_exp_probe", c_int, [c_float, c_float, c_float, c_void_p, c_void_p, c_void_p]),
    ("gsr_exp_probe2", c_int, [c_float, c_float, c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    ("gsr_alpha_cut_probe", c_int, [c_void_p, c_int, c_void_p]),
    ("gsr_rank_order_check", c_int, [POINTER(c_int64), POINTER(c_int64)]),
]

# C++-linkage drop-in loader (misc.cuh:4): mangled name of
# Gaussian* loadGaussianCudaFromPly(const std::string&, int*).
CXX_SYMBOLS = ["_Z23loadGaussianCudaFromPlyRKNSt7__cxx1112basic_stringIcSt11char_traitsIcESaIcEEEPi"]

_lib = None


def lib() -> ctypes.CDLL:
    """Load libgsr.so once; raises if it was not built (no fallback path)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: run `make` (or __graft_entry__.build()) first")
    L = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    for name, res, args in SIGNATURES:
        try:
            fn = getattr(L, name)
        except AttributeError:
            if os.environ.get("GSR_LIBRARY"):   # an older build in an A/B run: its API subset
                continue
            raise
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


class GsrError(RuntimeError):
    def __init__(self, code: int, where: str):
        msg = lib().gsr_last_error().decode(errors="replace")
        super().__init__(f"{where} failed ({code}): {msg}")
        self.code = code


def check(code: int, where: str) -> int:
    if code != GSR_OK:
        raise GsrError(code, where)
    return code
