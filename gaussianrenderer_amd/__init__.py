"""gaussianrenderer_amd — MI355X-native 3D Gaussian splatting rasterizer.

Host-side mirror of the reference's interface (wwangg22/GaussianRenderer):

* :func:`loadGaussianCudaFromPly`  — misc.cu:13-134 (device scene block)
* :func:`preprocessCUDAGaussians`  — render.cu:871-1157 (whole frame, host image)
* :func:`preprocessCUDAGaussiansGL` — Canvas::render (canvas.cpp:337-351) into the
  viewer's colour SSBO, no host round trip (include/gsr_gl.h; :class:`DisplayTarget`)
* :class:`TilingInformation`       — utils/gaussians.hpp:38-60
* :func:`make_camera` / :func:`orbit` — scene/camera.cpp

and the native stream-ordered API (:class:`Renderer`) used by the bench.
Everything that renders runs in libgsr.so (hand-written gfx950 HIP kernels);
there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
from ctypes import byref, c_float, c_int, c_int64, c_void_p

import numpy as np

from . import _native
from ._native import (AUX_MAX_FEATURES, AuxTargets, BackwardTargets, CONTRIB_WEIGHT_ONE, Camera, ContribTargets, GsrError, LAYOUT_AOS, LAYOUT_SCENE_BLOCK, LAYOUT_SCENE_BLOCK_4D,
                      LAYOUT_SCENE_BLOCK_SH3, NUM_STAGES, PLY_SH3, PLY_TYPED, SCENE4D_NARRAYS, SCENE_NARRAYS,
                      SCENE_SH3_NARRAYS, RecordGrads, SceneGrads, AuxUpstream, RecordGradsAux, RecordGradsAuxOut,
                      ADAM_OPACITY_MAX, ADAM_OPACITY_MIN, ADAM_SKIP_ZERO, ADAM_ZERO_GRADS, AdamConfig,
                      LOSS_NVALUES, LossConfig, DENSIFY_CHUNK,
                      InitConfig, KNN_BOUNDS_CHUNK, KNN_FAN, KNN_LEAF, KNN_SORT_TILE, SH_C0,
                      SPLAT_RECORD_BYTES, STAGES, TILE_PX, check, lib)

__all__ = [
    "Camera", "GsrError", "Renderer", "Scene", "TilingInformation", "make_camera", "orbit",
    "loadGaussianCudaFromPly", "preprocessCUDAGaussians", "read_ply", "write_synthetic_ply",
    "SPLAT_DTYPE", "STAGES", "TILE_PX", "lib", "AUX_MAX_FEATURES", "DisplayTarget", "display_gl_current", "preprocessCUDAGaussiansGL",
    "CONTRIB_WEIGHT_ONE", "ContribTargets", "BackwardTargets", "mask_indices", "gather_planes",
    "RecordGrads", "SceneGrads", "AuxUpstream", "RecordGradsAux", "RecordGradsAuxOut",
    "AdamConfig", "ADAM_SKIP_ZERO", "ADAM_ZERO_GRADS", "ADAM_OPACITY_MIN", "ADAM_OPACITY_MAX", "SCENE_GRAD_GROUPS",
    "LossConfig", "LOSS_NVALUES", "image_loss", "image_loss_scratch_bytes",
    "densify_accumulate", "densify_gather_planes", "densify_normals", "DENSIFY_CHUNK",
    "points_knn_scratch_bytes", "points_knn_dist2", "InitConfig", "KNN_LEAF", "KNN_FAN", "KNN_BOUNDS_CHUNK",
    "KNN_SORT_TILE", "SH_C0",
    "write_ply", "ply_row_floats", "raw_probe",
]

# gsr_read_splats record (include/gsr.h).
SPLAT_DTYPE = np.dtype([
    ("inv_covar", "<f4", 4), ("opacity", "<f4"), ("color", "<f4", 3),
    ("px_x", "<i4"), ("px_y", "<i4"), ("x_range", "<u4"), ("y_range", "<u4"),
    ("tile_x_range", "<u4"), ("tile_y_range", "<u4"), ("tile_count", "<u4"), ("depth_key", "<u4"),
])
assert SPLAT_DTYPE.itemsize == SPLAT_RECORD_BYTES


class TilingInformation:
    """utils/gaussians.hpp:38-60 — ctor argument order (ny, nx, h, w)."""

    def __init__(self, ny: int, nx: int, h: int, w: int):
        self.num_tile_y, self.num_tile_x, self.H, self.W = ny, nx, h, w
        self._strides()

    def _strides(self):
        self.width_stride = max(1, (self.W + self.num_tile_x - 1) // self.num_tile_x)
        self.height_stride = max(1, (self.H + self.num_tile_y - 1) // self.num_tile_y)

    def resize(self, h: int, w: int, num_tile_x: int, num_tile_y: int):
        self.H, self.W, self.num_tile_x, self.num_tile_y = h, w, num_tile_x, num_tile_y
        self._strides()


def make_camera(position=(0.0, 0.0, 4.0), look_at=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov_y=50.0,
                aspect=16.0 / 9.0, near=0.1, far=100.0) -> Camera:
    """Camera() + setters + updateCameraMatrices() + updateFrustumPlanes() (camera.cpp)."""
    cam = Camera()
    L = lib()
    L.gsr_camera_default(byref(cam))
    cam.position[:] = [float(v) for v in position]
    cam.lookAt[:] = [float(v) for v in look_at]
    cam.w_up[:] = [float(v) for v in up]
    cam.fovY, cam.aspectRatio, cam.nearClip, cam.farClip = fov_y, aspect, near, far
    L.gsr_camera_update(byref(cam))
    L.gsr_camera_update_frustum(byref(cam))
    return cam


def orbit(cam: Camera, azimuth_deg: float, elevation_deg: float = 0.0) -> Camera:
    """Camera::orbit (camera.cpp:130-158), in place; returns cam."""
    lib().gsr_camera_orbit(byref(cam), azimuth_deg, elevation_deg)
    return cam


def camera_intrinsics(cam: Camera):
    fx, fy = c_float(), c_float()
    lib().gsr_camera_intrinsics(byref(cam), byref(fx), byref(fy))
    return fx.value, fy.value


def read_ply(path: str, typed: bool = False, four_d: bool | None = False, sh3: bool = False) -> np.ndarray:
    """Host PLY parse -> (38, n) float32 SoA (reference loader semantics), or the
    hardened typed reader (typed=True: declared types, ascii, big-endian).
    four_d=True returns the (49, n) 4D arrays; four_d=None picks by the file;
    sh3=True the (59, n) "Inria-correct" degree-3 SH arrays."""
    L = lib()
    n = c_int64(-1)
    is4d = c_int(0)
    flags = (PLY_TYPED if typed else 0) | (PLY_SH3 if sh3 else 0)
    check(L.gsr_ply_read_host_ex(path.encode(), None, SCENE_SH3_NARRAYS if sh3 else SCENE_NARRAYS, 0, byref(n),
                                 flags, byref(is4d)), "gsr_ply_read_host")
    na = SCENE4D_NARRAYS if (four_d or (four_d is None and is4d.value)) else SCENE_NARRAYS
    if sh3:
        na = SCENE_SH3_NARRAYS
    soa = np.zeros((na, n.value), dtype=np.float32)
    check(L.gsr_ply_read_host_ex(path.encode(), soa.ctypes.data, na, n.value, byref(n), flags, None),
          "gsr_ply_read_host")
    return soa


def write_synthetic_ply(path: str, n: int, seed: int) -> None:
    """Seeded synthetic 62-property 3DGS PLY."""
    check(lib().gsr_synth_write_ply(path.encode(), int(n), int(seed)), "gsr_synth_write_ply")


def write_synthetic_ply4d(path: str, n: int, seed: int) -> None:
    """Seeded synthetic 4D (Spacetime-Gaussian style, 73-property) PLY for config 5."""
    check(lib().gsr_synth_write_ply4d(path.encode(), int(n), int(seed)), "gsr_synth_write_ply4d")


def write_ply(path: str, soa: np.ndarray) -> None:
    """A (38 | 49 | 59, n) float32 SoA, activated as read_ply and Scene.download give it, as a
    3DGS .ply (gsr_ply_write_host): the inverse of read_ply, and byte for byte what
    Scene.save_ply writes for the same values."""
    soa = np.ascontiguousarray(soa, dtype=np.float32)
    if soa.ndim != 2:
        raise ValueError("write_ply: soa must be (narrays, n)")
    check(lib().gsr_ply_write_host(str(path).encode(), soa.ctypes.data, soa.shape[0], soa.shape[1]),
          "gsr_ply_write_host")


def ply_row_floats(narrays: int) -> int:
    """Floats per row of the .ply of a block with `narrays` arrays: 62, or 73 for a 4D block."""
    p = int(lib().gsr_ply_row_floats(int(narrays)))
    if p < 0:
        raise GsrError(p, "gsr_ply_row_floats")
    return p


def raw_probe(x, kind: int) -> np.ndarray:
    """gsr_raw_log (kind 0) or gsr_raw_logit (kind 1) of float32 values on the host: the raw
    value the PLY writers store for a scale or an opacity."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.empty_like(x)
    check(lib().gsr_raw_probe(x.ctypes.data, x.size, int(kind), out.ctypes.data), "gsr_raw_probe")
    return out


class Scene:
    """A device scene block (one hipMalloc: header + SoA arrays)."""

    def __init__(self, ptr: int, n: int, owned: bool = True, narrays: int = SCENE_NARRAYS):
        self.ptr, self.n, self.owned, self.narrays = ptr, n, owned, narrays

    @property
    def is_4d(self) -> bool:
        return self.narrays == SCENE4D_NARRAYS

    @property
    def is_sh3(self) -> bool:
        return self.narrays == SCENE_SH3_NARRAYS

    @property
    def layout(self) -> int:
        return (LAYOUT_SCENE_BLOCK_4D if self.is_4d else LAYOUT_SCENE_BLOCK_SH3 if self.is_sh3
                else LAYOUT_SCENE_BLOCK)

    @classmethod
    def from_soa(cls, soa: np.ndarray) -> "Scene":
        soa = np.ascontiguousarray(soa, dtype=np.float32)
        assert soa.shape[0] in (SCENE_NARRAYS, SCENE4D_NARRAYS, SCENE_SH3_NARRAYS)
        ptr = lib().gsr_scene_upload_ex(soa.ctypes.data, soa.shape[0], soa.shape[1])
        if not ptr:
            raise GsrError(-2, "gsr_scene_upload")
        return cls(ptr, soa.shape[1], narrays=soa.shape[0])

    @classmethod
    def from_ply(cls, path: str, typed: bool = False, allow_4d: bool = True, sh3: bool = False) -> "Scene":
        """Device scene from a .ply (the reference loader unless typed=True); a file
        with the 4D properties loads as a 4D scene when allow_4d; sh3=True gives
        the "Inria-correct" degree-3 SH scene."""
        n = c_int(0)
        na = c_int(SCENE_NARRAYS)
        flags = (PLY_TYPED if typed else 0) | (PLY_SH3 if sh3 else 0)
        ptr = lib().gsr_load_ply_device_ex(path.encode(), byref(n), flags,
                                           byref(na) if (allow_4d or sh3) else None)
        if not ptr:
            raise GsrError(-3, f"loadGaussianCudaFromPly({path}): {lib().gsr_last_error().decode()}")
        return cls(ptr, n.value, narrays=na.value if (allow_4d or sh3) else SCENE_NARRAYS)

    @classmethod
    def from_points(cls, xyz_ptr, n: int, rgb_ptr=None, *, narrays: int = SCENE_NARRAYS, opacity: float = 0.1,
                    min_dist2: float = 1e-7, scale_mul: float = 1.0, scale_max: float = float("inf"),
                    t_center: float = 0.0, t_scale: float = 1.0, point_stride: int = 3, comp_stride: int = 1,
                    rgb_point_stride: int = 3, rgb_comp_stride: int = 1, mean2_ptr=None, bad_ptr=None,
                    stream: int = 0) -> "Scene":
        """A new owned scene from a device point cloud, as 3DGS's create_from_pcd starts one
        (gsr_scene_from_points, include/gsr.h): positions the points (n x 3 floats at xyz_ptr,
        coordinate c of point i at i * point_stride + c * comp_stride), SH dc from the colours
        in [0, 1] (rgb_ptr, the same addressing with its own strides; None: 0.5 grey), identity
        rotation, one stored opacity, and every scale min(sqrt(max(mean2, min_dist2)) *
        scale_mul, scale_max) with mean2 the exact mean squared distance to the point's three
        nearest neighbours.  mean2_ptr (optional, n floats) receives mean2; bad_ptr (optional
        device uint32; zero it first) counts the points with a non-finite coordinate, which
        are copied as they are and are nobody's neighbour.  t_center / t_scale: the stored
        temporal centre and scale of a 4D block.  Synchronous on `stream`."""
        xyz, rgb = _dev_ptr(xyz_ptr), _dev_ptr(rgb_ptr)
        if n > 0 and not xyz:
            raise ValueError("Scene.from_points: xyz_ptr is missing")
        if narrays not in (SCENE_NARRAYS, SCENE4D_NARRAYS, SCENE_SH3_NARRAYS):
            raise ValueError(f"Scene.from_points: narrays = {narrays}")
        cfg = InitConfig(float(opacity), float(min_dist2), float(scale_mul), float(scale_max), float(t_center),
                         float(t_scale), 0)
        ptr = lib().gsr_scene_from_points(xyz or None, int(point_stride), int(comp_stride), rgb or None,
                                          int(rgb_point_stride), int(rgb_comp_stride), int(n), int(narrays),
                                          byref(cfg), _dev_ptr(mean2_ptr) or None, _dev_ptr(bad_ptr) or None,
                                          stream or None)
        if not ptr:
            raise GsrError(_native.GSR_E_ARG, "gsr_scene_from_points")
        return cls(ptr, int(n), narrays=int(narrays))

    def knn_dist2(self, out_ptr, scratch_ptr, scratch_bytes: int, bad_ptr=None, stream: int = 0) -> None:
        """points_knn_dist2() on this block's own positions (its x, y, z arrays, planar with the
        block's stride), stream-ordered: out_ptr receives n floats."""
        if not self.ptr and self.n > 0:
            raise ValueError("Scene.knn_dist2: the scene has been freed")
        stride = (self.n + 63) // 64 * 64
        points_knn_dist2(self.ptr + _native.SCENE_HEADER_BYTES if self.ptr else None, self.n, out_ptr, scratch_ptr,
                         scratch_bytes, point_stride=1, comp_stride=max(stride, 2), bad_ptr=bad_ptr, stream=stream)

    def download(self) -> np.ndarray:
        soa = np.zeros((self.narrays, self.n), dtype=np.float32)
        check(lib().gsr_scene_download(self.ptr, soa.ctypes.data, self.n), "gsr_scene_download")
        return soa

    def select(self, keep_ptr, indices_ptr=None, stream: int = 0) -> "Scene":
        """A new owned scene of the Gaussians whose byte in the device mask keep_ptr (n uint8,
        any non-zero value keeps) is set, in index order, built on the device
        (gsr_scene_select, include/gsr.h); its .n is the kept count.  indices_ptr (optional,
        room for n int32) receives the kept source indices, for gather_planes() on side
        arrays.  Synchronous on `stream`."""
        keep = _dev_ptr(keep_ptr)
        if not keep and self.n > 0:
            raise ValueError("Scene.select: keep_ptr is missing")
        m = c_int64(-1)
        ptr = lib().gsr_scene_select(self.ptr, self.narrays, self.n, keep or None, byref(m),
                                     _dev_ptr(indices_ptr) or None, stream or None)
        if not ptr:
            raise GsrError(_native.GSR_E_ARG, "gsr_scene_select")
        return Scene(ptr, int(m.value), narrays=self.narrays)

    def gather(self, indices_ptr, m: int, bad_ptr=None, stream: int = 0) -> "Scene":
        """A new owned scene of m Gaussians, Gaussian j being this scene's Gaussian
        indices[j] (device int32, any order, repeats allowed), stream-ordered
        (gsr_scene_gather).  An index outside [0, n) reads the nearest valid Gaussian and
        counts into the device uint32 bad_ptr (optional; zero it first)."""
        idx = _dev_ptr(indices_ptr)
        if not idx and m > 0:
            raise ValueError("Scene.gather: indices_ptr is missing")
        ptr = lib().gsr_scene_gather(self.ptr, self.narrays, self.n, idx or None, int(m),
                                     _dev_ptr(bad_ptr) or None, stream or None)
        if not ptr:
            raise GsrError(_native.GSR_E_ARG, "gsr_scene_gather")
        return Scene(ptr, int(m), narrays=self.narrays)

    def adam_step(self, grads, m, v, *, step: int, lr_position: float = 0.0, lr_opacity: float = 0.0,
                  lr_scale: float = 0.0, lr_rot: float = 0.0, lr_sh_dc: float = 0.0, lr_sh_rest: float = 0.0,
                  lr_tcenter: float = 0.0, lr_tscale: float = 0.0, lr_motion: float = 0.0, beta1: float = 0.9,
                  beta2: float = 0.999, eps: float = 1e-15, skip_zero: bool = False, zero_grads: bool = False,
                  bad_ptr=None, stream: int = 0) -> None:
        """One fused in-place Adam step of this block on the device (gsr_scene_adam_step,
        include/gsr.h), stream-ordered: with reset_opacity() the only call that writes to a scene block.  grads (what
        project_backward / render_backward_scene accumulated), m and v (the moments: same
        shapes, float32 planar [c*n + i], zeroed once by the caller) each name up to six device
        buffers: a dict with keys from SCENE_GRAD_GROUPS ("position" 3 planes, "opacity" 1,
        "scale" 3, "rot" 4, "sh" 27 or 48, "temporal" 11; a missing key is None), a sequence of
        six in that order, or a SceneGrads; every pointer an int, anything with .data_ptr(), or
        None.  A group is stepped when its gradient is given and its lr is not 0 (lr_sh_dc:
        the first 3 sh planes, lr_sh_rest: the others; lr_tcenter, lr_tscale, lr_motion: plane
        0, plane 1, planes 2..10 of "temporal"); a frozen group is neither read nor written.
        The opacity, the scales and trbf_scale are stepped in raw (logit / log) space.  step:
        the 1-based iteration, for the bias correction.  skip_zero: elements with a zero
        gradient keep x, m and v (the visible-only step); zero_grads: the active gradient planes
        are zero afterwards.  Elements with a non-finite gradient are skipped and counted into
        the device uint32 bad_ptr (optional; zero it first)."""
        gs, ms, vs = (_scene_grads(p, name) for p, name in ((grads, "grads"), (m, "m"), (v, "v")))
        lrs = (lr_position, lr_opacity, lr_scale, lr_rot, lr_sh_dc, lr_sh_rest, lr_tcenter, lr_tscale, lr_motion)
        active = False
        for (field, _), glrs in zip(SceneGrads._fields_, (lrs[0:1], lrs[1:2], lrs[2:3], lrs[3:4], lrs[4:6], lrs[6:9])):
            if getattr(gs, field) and any(lr != 0 for lr in glrs):
                active = True
                if not (getattr(ms, field) and getattr(vs, field)):
                    raise ValueError(f"Scene.adam_step: {field} is stepped but its m or v pointer is missing")
        if not active:
            raise ValueError("Scene.adam_step: no group to step (a gradient pointer with a non-zero lr)")
        if not self.ptr and self.n > 0:
            raise ValueError("Scene.adam_step: the scene has been freed")
        cfg = _native.AdamConfig(*[float(lr) for lr in lrs], float(beta1), float(beta2), float(eps), int(step),
                                 (ADAM_SKIP_ZERO if skip_zero else 0) | (ADAM_ZERO_GRADS if zero_grads else 0))
        check(lib().gsr_scene_adam_step(self.ptr or None, self.layout, self.n, byref(gs), byref(ms), byref(vs),
                                        byref(cfg), _dev_ptr(bad_ptr) or None, stream or None), "gsr_scene_adam_step")

    def densify(self, grad_accum_ptr, seen_ptr, *, grad_threshold: float = 0.0002, scale_split: float,
                min_opacity: float = 0.005, prune_scale_max: float = float("inf"), split_shrink: float = 1.6,
                seed: int = 0, src_ptr=None, kind_ptr=None, stream: int = 0):
        """3DGS's adaptive density control on the device (gsr_scene_densify, include/gsr.h):
        returns (a new owned Scene, report dict).  grad_accum_ptr / seen_ptr: the statistic
        densify_accumulate() summed (n floats / n uint32).  A Gaussian whose accum / seen
        reaches grad_threshold is cloned when its largest scale is <= scale_split and split
        into two children (scales / split_shrink, positions drawn from the parent under
        `seed`) when it is larger; outputs whose opacity is below min_opacity or whose largest
        scale exceeds prune_scale_max are dropped.  src_ptr (optional, room for 2n int32) and
        kind_ptr (optional, room for 2n uint8) receive every output's source index and kind (0
        the source itself, 1 its clone, 2 and 3 the children), for densify_gather_planes().
        The report counts the sources: n_out, kept, cloned, split, pruned.  Synchronous on
        `stream`."""
        accum, seen = _dev_ptr(grad_accum_ptr), _dev_ptr(seen_ptr)
        if self.n > 0 and not (accum and seen):
            raise ValueError("Scene.densify: grad_accum_ptr / seen_ptr is missing")
        cfg = _native.DensifyConfig(float(grad_threshold), float(scale_split), float(min_opacity),
                                    float(prune_scale_max), float(split_shrink), int(seed) & (2 ** 64 - 1), 0)
        rep = _native.DensifyReport()
        ptr = lib().gsr_scene_densify(self.ptr or None, self.narrays, self.n, accum or None, seen or None, byref(cfg),
                                      _dev_ptr(src_ptr) or None, _dev_ptr(kind_ptr) or None, byref(rep),
                                      stream or None)
        if not ptr:
            raise GsrError(_native.GSR_E_ARG, "gsr_scene_densify")
        report = {name: int(getattr(rep, name)) for name, _ in _native.DensifyReport._fields_}
        return Scene(ptr, report["n_out"], narrays=self.narrays), report

    def reset_opacity(self, cap: float = 0.01, m_opacity_ptr=None, v_opacity_ptr=None, stream: int = 0) -> None:
        """3DGS's periodic opacity reset, in place and stream-ordered (gsr_scene_reset_opacity):
        every stored opacity becomes min(opacity, cap) and the opacity group's two Adam moment
        planes (optional, n floats each) are zeroed."""
        if not self.ptr and self.n > 0:
            raise ValueError("Scene.reset_opacity: the scene has been freed")
        check(lib().gsr_scene_reset_opacity(self.ptr or None, self.layout, self.n, float(cap),
                                            _dev_ptr(m_opacity_ptr) or None, _dev_ptr(v_opacity_ptr) or None,
                                            stream or None), "gsr_scene_reset_opacity")

    def save_ply(self, path: str, chunk_rows: int = 0, stream: int = 0) -> None:
        """This block as a 3DGS .ply (gsr_scene_save_ply, include/gsr.h "scene export"): the
        inverse of from_ply, byte-identical to write_ply(path, self.download()).  The rows are
        de-activated and interleaved on the device and streamed out in chunks of chunk_rows
        rows (0: 65,536) through pinned buffers; the file appears under `path` only when it is
        complete.  Synchronous on `stream`: work queued there before the call is in the file."""
        if not self.ptr:
            raise ValueError("Scene.save_ply: the scene has been freed")
        check(lib().gsr_scene_save_ply(self.ptr, self.narrays, self.n, str(path).encode(), int(chunk_rows),
                                       stream or None), "gsr_scene_save_ply")

    def pack_rows(self, out_ptr, first: int, count: int, stream: int = 0) -> None:
        """Rows [first, first + count) of this block in the .ply row format into the device
        floats at out_ptr (count * ply_row_floats(narrays) of them; nothing past them is
        written), stream-ordered (gsr_scene_pack_rows)."""
        out = _dev_ptr(out_ptr)
        if count > 0 and not out:
            raise ValueError("Scene.pack_rows: out_ptr is missing")
        if count > 0 and not self.ptr:
            raise ValueError("Scene.pack_rows: the scene has been freed")
        check(lib().gsr_scene_pack_rows(self.ptr or None, self.layout, self.n, int(first), int(count), out or None,
                                        stream or None), "gsr_scene_pack_rows")

    def free(self):
        if self.ptr and self.owned:
            lib().gsr_scene_free(self.ptr)
        self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _dev_ptr(p) -> int:
    """A device address from an int or anything with .data_ptr() (a torch tensor); None -> 0."""
    if p is None:
        return 0
    return int(p.data_ptr()) if hasattr(p, "data_ptr") else int(p)


# the pointers of a SceneGrads, in the block's array order
SCENE_GRAD_GROUPS = ("position", "opacity", "scale", "rot", "sh", "temporal")


def _scene_grads(p, what: str) -> SceneGrads:
    """A SceneGrads from a SceneGrads, a dict keyed by SCENE_GRAD_GROUPS or a sequence of six
    pointers (ints, anything with .data_ptr(), or None)."""
    if isinstance(p, SceneGrads):
        return p
    if p is None:
        raise ValueError(f"Scene.adam_step: {what} is missing")
    if isinstance(p, dict):
        unknown = set(p) - set(SCENE_GRAD_GROUPS)
        if unknown:
            raise ValueError(f"Scene.adam_step: {what} has unknown groups {sorted(unknown)}")
        vals = [p.get(k) for k in SCENE_GRAD_GROUPS]
    else:
        vals = list(p)
        if len(vals) != len(SCENE_GRAD_GROUPS):
            raise ValueError(f"Scene.adam_step: {what} needs {len(SCENE_GRAD_GROUPS)} pointers ({SCENE_GRAD_GROUPS})")
    return SceneGrads(*[_dev_ptr(x) or None for x in vals])


def mask_indices(keep_ptr, n: int, indices_ptr, stream: int = 0) -> int:
    """Stable compaction of a device keep mask (gsr_mask_indices): writes the ascending indices
    i < n whose mask byte is non-zero into the device int32 array indices_ptr (room for n;
    words past the count are untouched) and returns their number.  Synchronous on `stream`."""
    keep, idx = _dev_ptr(keep_ptr), _dev_ptr(indices_ptr)
    if n > 0 and not keep:
        raise ValueError("mask_indices: keep_ptr is missing")
    if n > 0 and not idx:
        raise ValueError("mask_indices: indices_ptr is missing")
    m = c_int64(-1)
    check(lib().gsr_mask_indices(keep or None, int(n), idx or None, byref(m), stream or None), "gsr_mask_indices")
    return int(m.value)


def gather_planes(dst_ptr, dst_stride: int, src_ptr, src_stride: int, nplanes: int, elem_bytes: int, n: int,
                  indices_ptr, m: int, bad_ptr=None, stream: int = 0) -> None:
    """dst[p*dst_stride + j] = src[p*src_stride + indices[j]] for p < nplanes, j < m, on the
    device, stream-ordered (gsr_gather_planes): elements of 4 or 8 bytes copied as bits,
    strides in elements.  An index outside [0, n) reads the nearest valid element and counts
    into the device uint32 bad_ptr (optional; zero it first)."""
    dst, src, idx = _dev_ptr(dst_ptr), _dev_ptr(src_ptr), _dev_ptr(indices_ptr)
    if not idx:
        raise ValueError("gather_planes: indices_ptr is missing")
    if not (dst and src):
        raise ValueError("gather_planes: dst_ptr / src_ptr is missing")
    check(lib().gsr_gather_planes(dst, int(dst_stride), src, int(src_stride), int(nplanes), int(elem_bytes),
                                  int(n), idx, int(m), _dev_ptr(bad_ptr) or None, stream or None),
          "gsr_gather_planes")


def densify_accumulate(center_ptr, n: int, W: int, H: int, grad_accum_ptr, seen_ptr, bad_ptr=None,
                       stream: int = 0) -> None:
    """The densification statistic of one backward frame, on the device and stream-ordered
    (gsr_densify_accumulate): center_ptr names the two centre planes of render_backward
    (center_ptr) or planes 8 and 9 of render_backward_scene's record scratch; every Gaussian a
    pixel composited adds the norm of its centre gradient in NDC units to grad_accum_ptr (n
    floats) and 1 to seen_ptr (n uint32).  Non-finite entries are skipped and counted into the
    device uint32 bad_ptr (optional; zero it first)."""
    center, accum, seen = _dev_ptr(center_ptr), _dev_ptr(grad_accum_ptr), _dev_ptr(seen_ptr)
    if n > 0 and not (center and accum and seen):
        raise ValueError("densify_accumulate: center_ptr / grad_accum_ptr / seen_ptr is missing")
    check(lib().gsr_densify_accumulate(center or None, int(n), int(W), int(H), accum or None, seen or None,
                                       _dev_ptr(bad_ptr) or None, stream or None), "gsr_densify_accumulate")


def densify_gather_planes(dst_ptr, dst_stride: int, src_ptr, src_stride: int, nplanes: int, n: int, indices_ptr,
                          kind_ptr, m: int, bad_ptr=None, stream: int = 0) -> None:
    """dst[p*dst_stride + j] = 0 if kind[j] else src[p*src_stride + indices[j]] over float
    planes, on the device, stream-ordered (gsr_densify_gather_planes): cuts the Adam moments
    over to the scene Scene.densify() returned, through the lists it wrote — survivors keep
    their moments, every new Gaussian starts at zero."""
    dst, src, idx, kind = _dev_ptr(dst_ptr), _dev_ptr(src_ptr), _dev_ptr(indices_ptr), _dev_ptr(kind_ptr)
    if not (idx and kind):
        raise ValueError("densify_gather_planes: indices_ptr / kind_ptr is missing")
    if not (dst and src):
        raise ValueError("densify_gather_planes: dst_ptr / src_ptr is missing")
    check(lib().gsr_densify_gather_planes(dst, int(dst_stride), src, int(src_stride), int(nplanes), int(n), idx, kind,
                                          int(m), _dev_ptr(bad_ptr) or None, stream or None),
          "gsr_densify_gather_planes")


def points_knn_scratch_bytes(n: int) -> int:
    """Bytes of device scratch points_knn_dist2() needs for n points (about 32 n)."""
    b = int(lib().gsr_points_knn_scratch_bytes(int(n)))
    if b < 0:
        raise GsrError(b, "gsr_points_knn_scratch_bytes")
    return b


def points_knn_dist2(xyz_ptr, n: int, out_ptr, scratch_ptr, scratch_bytes: int, *, point_stride: int = 3,
                     comp_stride: int = 1, bad_ptr=None, stream: int = 0) -> None:
    """out[i] = the mean squared distance from point i to its three nearest neighbours, exact
    in float32 and reproducible bit for bit, on the device and stream-ordered
    (gsr_points_knn_dist2, include/gsr.h): what 3DGS initialises its scales from.  Coordinate c
    of point i is at xyz_ptr[i * point_stride + c * comp_stride] (floats): (3, 1) an interleaved
    [n, 3] tensor, (1, S) planar.  Points with a non-finite coordinate are nobody's neighbour,
    get 0 and count into the device uint32 bad_ptr (optional; zero it first).  scratch_ptr:
    points_knn_scratch_bytes(n) bytes of device memory, the call's only working memory."""
    xyz, out, scratch = _dev_ptr(xyz_ptr), _dev_ptr(out_ptr), _dev_ptr(scratch_ptr)
    if n > 0 and not (xyz and out):
        raise ValueError("points_knn_dist2: xyz_ptr / out_ptr is missing")
    if n > 0 and not scratch:
        raise ValueError("points_knn_dist2: scratch_ptr is missing")
    check(lib().gsr_points_knn_dist2(xyz or None, int(point_stride), int(comp_stride), int(n), out or None,
                                     _dev_ptr(bad_ptr) or None, scratch or None, max(int(scratch_bytes), 0),
                                     stream or None), "gsr_points_knn_dist2")


def densify_normals(seed: int, index, child) -> np.ndarray:
    """The split sampler on the host (gsr_densify_normals): the three float32 normals of child
    `child` of source `index` under `seed`, bit for bit what the split kernel draws; index and
    child may be equal-length arrays (the result is then (len, 3))."""
    idx, ch = np.atleast_1d(np.asarray(index, np.uint32)), np.atleast_1d(np.asarray(child, np.uint32))
    idx, ch = np.broadcast_arrays(idx, ch)
    out = np.zeros((idx.size, 3), np.float32)
    f, base, s = lib().gsr_densify_normals, out.ctypes.data, int(seed) & (2 ** 64 - 1)
    for j, (i, k) in enumerate(zip(idx.tolist(), ch.tolist())):
        f(s, i, k, base + 12 * j)
    return out if np.ndim(index) or np.ndim(child) else out[0]


def image_loss_scratch_bytes(W: int, H: int, want_grad: bool = True) -> int:
    """Bytes of device scratch gsr_image_loss needs for a W x H frame, with or without a
    gradient (gsr_image_loss_scratch_bytes)."""
    nbytes = lib().gsr_image_loss_scratch_bytes(int(W), int(H), 1 if want_grad else 0)
    if nbytes < 0:
        raise GsrError(int(nbytes), "gsr_image_loss_scratch_bytes")
    return int(nbytes)


def image_loss(image_ptr, target_ptr, W: int, H: int, *, w_l1: float = 0.8, w_l2: float = 0.0, w_dssim: float = 0.2,
               grad_scale: float = 1.0, grad_ptr=None, loss_ptr=None, scratch_ptr, scratch_bytes: int | None = None,
               stream: int = 0) -> None:
    """The 3DGS training loss of a rendered frame against its target on the device, stream-
    ordered (gsr_image_loss): w_l1 mean|x - y| + w_l2 mean (x - y)^2 + w_dssim (1 - mean SSIM).
    grad_ptr (3*W*H floats, overwritten) receives grad_scale * dL/d image, the grad_image of
    Renderer.render_backward_scene; loss_ptr (LOSS_NVALUES floats, overwritten) receives
    {L, mean|x - y|, mean (x - y)^2, mean SSIM}.  At least one of the two.  scratch_ptr: device
    memory of image_loss_scratch_bytes(W, H, grad_ptr is not None) bytes; scratch_bytes: what
    it really holds (default: exactly that)."""
    image, target, scratch = _dev_ptr(image_ptr), _dev_ptr(target_ptr), _dev_ptr(scratch_ptr)
    grad, loss = _dev_ptr(grad_ptr), _dev_ptr(loss_ptr)
    if not (image and target):
        raise ValueError("image_loss: image_ptr / target_ptr is missing")
    if not (grad or loss):
        raise ValueError("image_loss: neither grad_ptr nor loss_ptr is given")
    if not scratch:
        raise ValueError("image_loss: scratch_ptr is missing")
    if scratch_bytes is None:
        scratch_bytes = image_loss_scratch_bytes(W, H, bool(grad))
    cfg = LossConfig(float(w_l1), float(w_l2), float(w_dssim), float(grad_scale), 0)
    check(lib().gsr_image_loss(image, target, int(W), int(H), byref(cfg), grad or None, loss or None, scratch,
                               int(scratch_bytes), stream or None), "gsr_image_loss")


def loadGaussianCudaFromPly(path: str):
    """misc.cu:13-134 -> (device pointer or 0, numGaussians)."""
    n = c_int(0)
    ptr = lib().gsr_load_ply_device(path.encode(), byref(n))
    return (ptr or 0), n.value


def preprocessCUDAGaussians(d_gaussians: int, num_gaussians: int, cam: Camera, num_tile_y: int, num_tile_x: int,
                            width_stride: int, height_stride: int, tile_W: int, tile_H: int,
                            k: float, out: np.ndarray = None) -> np.ndarray:
    """render.cu:871-1157 through the drop-in C symbol; returns the host image (3, H, W).

    `out`: optional persistent C-contiguous float32 (3, H, W) host image to render
    into (the reference viewer's loop reuses one host buffer the same way)."""
    if out is None:
        out = np.zeros((3, tile_H, tile_W), dtype=np.float32)
    elif out.dtype != np.float32 or out.shape != (3, tile_H, tile_W) or not out.flags.c_contiguous:
        raise ValueError(f"out must be C-contiguous float32 (3, {tile_H}, {tile_W})")
    lib().preprocessCUDAGaussians(d_gaussians, out.ctypes.data_as(ctypes.POINTER(c_float)), num_gaussians, cam,
                                  num_tile_y, num_tile_x, width_stride, height_stride, tile_W, tile_H, k)
    return out


def display_gl_current() -> bool:
    """True if a GL context (GLX or EGL) is current on this thread."""
    return bool(lib().gsr_display_gl_current())


class DisplayTarget:
    """Where a frame is displayed (include/gsr_gl.h): the viewer's colour SSBO
    registered with HIP (`from_gl`), or device memory such as an imported
    Vulkan buffer (`from_device`).  The render writes it in place."""

    def __init__(self, ptr: int):
        self.ptr = ptr

    @classmethod
    def from_gl(cls, gl_buffer: int) -> "DisplayTarget":
        p = c_void_p()
        check(lib().gsr_display_register_gl(int(gl_buffer), byref(p)), "gsr_display_register_gl")
        return cls(p.value)

    @classmethod
    def from_device(cls, d_ptr: int, nbytes: int) -> "DisplayTarget":
        p = c_void_p()
        check(lib().gsr_display_wrap_device(d_ptr, int(nbytes), byref(p)), "gsr_display_wrap_device")
        return cls(p.value)

    def free(self):
        if self.ptr:
            p, self.ptr = self.ptr, 0
            check(lib().gsr_display_free(p), "gsr_display_free")

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def preprocessCUDAGaussiansGL(d_gaussians: int, gl_buffer: int, num_gaussians: int, cam: Camera, num_tile_y: int,
                              num_tile_x: int, width_stride: int, height_stride: int, tile_W: int, tile_H: int,
                              k: float) -> None:
    """Canvas::render (canvas.cpp:337-342) into the colour SSBO, no host round trip
    (include/gsr_gl.h).  Needs the viewer's GL context current on this thread."""
    lib().preprocessCUDAGaussiansGL(d_gaussians, int(gl_buffer), num_gaussians, cam, num_tile_y, num_tile_x,
                                    width_stride, height_stride, tile_W, tile_H, k)


def _event_handle(ev, wait: bool = False):
    """hipEvent_t of a torch.cuda.Event, or of a raw integer handle; None -> NULL.
    An event the library records into (wait=False) is created on first use (torch
    creates the HIP event lazily, at its first record).  A wait event that was never
    recorded has nothing to wait for: NULL (recording it here would make the lane wait
    on all work queued on torch's current stream, an implicit fork)."""
    if ev is None:
        return None
    if isinstance(ev, int):
        return ev
    if not ev.cuda_event:
        if wait:
            return None
        ev.record()
    return ev.cuda_event


class Renderer:
    """Persistent render context (stream-ordered, device-resident)."""

    def __init__(self):
        self.ctx = lib().gsr_create()

    def close(self):
        if self.ctx:
            lib().gsr_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reserve(self, n: int, pairs: int):
        check(lib().gsr_reserve(self.ctx, n, pairs), "gsr_reserve")

    def render(self, scene, cam: Camera, W: int, H: int, out_ptr: int, k: float = 3.0, tiling=None,
               stream: int = 0, layout: int = LAYOUT_SCENE_BLOCK, n: int | None = None,
               time: float | None = None) -> int:
        """Enqueue one frame into the device buffer out_ptr (3*W*H float32).
        4D scenes render at `time` (or the last gsr_set_time value).

        Returns GSR_OK, or GSR_E_OVERFLOW when an earlier frame overflowed the
        pair buffer (it has been grown; that frame must be re-rendered)."""
        ptr = scene.ptr if isinstance(scene, Scene) else int(scene)
        n = scene.n if n is None else n
        if isinstance(scene, Scene) and layout == LAYOUT_SCENE_BLOCK:
            layout = scene.layout
        if time is not None:
            self.set_time(time)
        t = tiling or TilingInformation(1, 1, H, W)
        rc = lib().gsr_render(self.ctx, ptr, layout, n, byref(cam), W, H, t.num_tile_x, t.num_tile_y,
                              t.width_stride, t.height_stride, k, out_ptr, stream or None)
        if rc not in (_native.GSR_OK, _native.GSR_E_OVERFLOW):
            raise GsrError(rc, "gsr_render")
        return rc

    def render_aux(self, scene, cam: Camera, W: int, H: int, out_ptr: int | None = None,
                   alpha_ptr: int | None = None, depth_ptr: int | None = None, features_ptr: int | None = None,
                   nfeat: int = 0, feat_out_ptr: int | None = None, k: float = 3.0, tiling=None, stream: int = 0,
                   layout: int = LAYOUT_SCENE_BLOCK, n: int | None = None, time: float | None = None) -> int:
        """Enqueue one frame with auxiliary targets (gsr_render_aux, include/gsr.h), each a
        device buffer or None: out_ptr the image (3*W*H float32, the exact blend's),
        alpha_ptr the accumulated alpha (W*H), depth_ptr the un-normalised depth sum (W*H;
        the expected depth is depth / alpha), and feat_out_ptr nfeat*W*H floats composited
        from features_ptr (nfeat arrays of n floats, feature f of Gaussian i at [f*n + i]).
        Same returns as render()."""
        nfeat = int(nfeat)
        if not 0 <= nfeat <= AUX_MAX_FEATURES:
            raise ValueError(f"render_aux: nfeat must be 0..{AUX_MAX_FEATURES}")
        if nfeat and not (features_ptr and feat_out_ptr):
            raise ValueError("render_aux: nfeat > 0 needs features_ptr and feat_out_ptr")
        if not nfeat and (features_ptr or feat_out_ptr):
            raise ValueError("render_aux: features_ptr / feat_out_ptr given with nfeat = 0")
        if not (out_ptr or alpha_ptr or depth_ptr or nfeat):
            raise ValueError("render_aux: no output requested")
        ptr = scene.ptr if isinstance(scene, Scene) else int(scene)
        n = scene.n if n is None else n
        if isinstance(scene, Scene) and layout == LAYOUT_SCENE_BLOCK:
            layout = scene.layout
        if time is not None:
            self.set_time(time)
        t = tiling or TilingInformation(1, 1, H, W)
        aux = AuxTargets(alpha_ptr or None, depth_ptr or None, features_ptr or None, nfeat, feat_out_ptr or None)
        rc = lib().gsr_render_aux(self.ctx, ptr, layout, n, byref(cam), W, H, t.num_tile_x, t.num_tile_y,
                                  t.width_stride, t.height_stride, k, out_ptr or None, byref(aux), stream or None)
        if rc not in (_native.GSR_OK, _native.GSR_E_OVERFLOW):
            raise GsrError(rc, "gsr_render_aux")
        return rc

    def render_contrib(self, scene, cam: Camera, W: int, H: int, count_ptr: int | None = None,
                       weight_ptr: int | None = None, max_ptr: int | None = None, id_ptr: int | None = None,
                       k: float = 3.0, tiling=None, stream: int = 0, layout: int = LAYOUT_SCENE_BLOCK,
                       n: int | None = None, time: float | None = None) -> int:
        """Enqueue one frame of contribution statistics (gsr_render_contrib, include/gsr.h), each
        a device buffer or None.  Per Gaussian, ACCUMULATED (zero them once; every frame adds):
        count_ptr n uint32, the pixels that composited it; weight_ptr n uint64, the sum of their
        blend weights in fixed point (CONTRIB_WEIGHT_ONE = 1.0); max_ptr n uint32, the float
        bits of its largest weight.  id_ptr W*H int32, overwritten: per pixel the composited
        Gaussian with the largest weight, -1 for none.  A frame that overflows adds nothing.
        Same returns as render()."""
        if not (count_ptr or weight_ptr or max_ptr or id_ptr):
            raise ValueError("render_contrib: no output requested")
        ptr = scene.ptr if isinstance(scene, Scene) else int(scene)
        n = scene.n if n is None else n
        if isinstance(scene, Scene) and layout == LAYOUT_SCENE_BLOCK:
            layout = scene.layout
        if time is not None:
            self.set_time(time)
        t = tiling or TilingInformation(1, 1, H, W)
        out = ContribTargets(count_ptr or None, weight_ptr or None, max_ptr or None, id_ptr or None)
        rc = lib().gsr_render_contrib(self.ctx, ptr, layout, n, byref(cam), W, H, t.num_tile_x, t.num_tile_y,
                                      t.width_stride, t.height_stride, k, byref(out), stream or None)
        if rc not in (_native.GSR_OK, _native.GSR_E_OVERFLOW):
            raise GsrError(rc, "gsr_render_contrib")
        return rc

    def render_backward(self, scene, cam: Camera, W: int, H: int, grad_image_ptr=None, grad_alpha_ptr=None,
                        color_ptr=None, opacity_ptr=None, conic_ptr=None, center_ptr=None, k: float = 3.0,
                        tiling=None, stream: int = 0, layout: int = LAYOUT_SCENE_BLOCK, n: int | None = None,
                        time: float | None = None) -> int:
        """Enqueue one frame of the blend's backward pass (gsr_render_backward, include/gsr.h);
        every pointer an int, anything with .data_ptr(), or None.  Inputs, at least one:
        grad_image_ptr 3*W*H float32 (dL/d image) and grad_alpha_ptr W*H (dL/d accumulated alpha).
        Outputs, at least one, float32, planar [c*n + i] and ACCUMULATED (zero them once; every
        frame adds): color_ptr 3 planes, opacity_ptr 1, conic_ptr 4 (inv_covar[0..3]), center_ptr 2
        (px_x, px_y): the gradients with respect to each Gaussian's splat record.  Summed with
        float atomics: not reproducible in the last bits.  A frame that overflows adds nothing.
        Same returns as render()."""
        gi, ga = _dev_ptr(grad_image_ptr), _dev_ptr(grad_alpha_ptr)
        outs = [_dev_ptr(p) for p in (color_ptr, opacity_ptr, conic_ptr, center_ptr)]
        if not (gi or ga):
            raise ValueError("render_backward: no upstream gradient given")
        if not any(outs):
            raise ValueError("render_backward: no output requested")
        ptr = scene.ptr if isinstance(scene, Scene) else int(scene)
        n = scene.n if n is None else n
        if isinstance(scene, Scene) and layout == LAYOUT_SCENE_BLOCK:
            layout = scene.layout
        if time is not None:
            self.set_time(time)
        t = tiling or TilingInformation(1, 1, H, W)
        bw = BackwardTargets(gi or None, ga or None, *[o or None for o in outs])
        rc = lib().gsr_render_backward(self.ctx, ptr, layout, n, byref(cam), W, H, t.num_tile_x, t.num_tile_y,
                                       t.width_stride, t.height_stride, k, byref(bw), stream or None)
        if rc not in (_native.GSR_OK, _native.GSR_E_OVERFLOW):
            raise GsrError(rc, "gsr_render_backward")
        return rc

    def project_backward(self, scene, cam: Camera, W: int, H: int, d_color_ptr=None, d_opacity_ptr=None,
                         d_conic_ptr=None, d_center_ptr=None, position_ptr=None, opacity_ptr=None, scale_ptr=None,
                         rot_ptr=None, sh_ptr=None, temporal_ptr=None, k: float = 3.0, stream: int = 0,
                         layout: int = LAYOUT_SCENE_BLOCK, n: int | None = None, time: float | None = None) -> int:
        """Enqueue the projection's backward pass (gsr_project_backward, include/gsr.h): the record
        gradients render_backward produced, carried on to the scene arrays; every pointer an int,
        anything with .data_ptr(), or None.  Inputs, at least one, float32 planar [c*n + i], None
        = zeros: d_color_ptr 3 planes, d_opacity_ptr 1, d_conic_ptr 4, d_center_ptr 2.  Outputs, at
        least one, planar [c*n + i] and ACCUMULATED: position_ptr 3 planes, opacity_ptr 1, scale_ptr
        3, rot_ptr 4, sh_ptr 27 (48 for an SH-3 scene), temporal_ptr 11 (4D scenes only), with
        respect to the stored (activated) values.  Gaussians with no record or an all-zero
        upstream are not touched.  No atomics: reproducible bit for bit.  The context's last
        frame (readbacks, timing, the depth split's controller) is left as it was."""
        ins = [_dev_ptr(p) for p in (d_color_ptr, d_opacity_ptr, d_conic_ptr, d_center_ptr)]
        outs = [_dev_ptr(p) for p in (position_ptr, opacity_ptr, scale_ptr, rot_ptr, sh_ptr, temporal_ptr)]
        if not any(ins):
            raise ValueError("project_backward: no upstream gradient given")
        if not any(outs):
            raise ValueError("project_backward: no output requested")
        ptr = scene.ptr if isinstance(scene, Scene) else int(scene)
        n = scene.n if n is None else n
        if isinstance(scene, Scene) and layout == LAYOUT_SCENE_BLOCK:
            layout = scene.layout
        if time is not None:
            self.set_time(time)
        rg = RecordGrads(*[p or None for p in ins])
        sg = SceneGrads(*[p or None for p in outs])
        check(lib().gsr_project_backward(self.ctx, ptr, layout, n, byref(cam), W, H, k, byref(rg), byref(sg),
                                         stream or None), "gsr_project_backward")
        return _native.GSR_OK

    def render_backward_scene(self, scene, cam: Camera, W: int, H: int, grad_image_ptr=None, grad_alpha_ptr=None,
                              scratch_ptr=None, position_ptr=None, opacity_ptr=None, scale_ptr=None, rot_ptr=None,
                              sh_ptr=None, temporal_ptr=None, k: float = 3.0, tiling=None, stream: int = 0,
                              layout: int = LAYOUT_SCENE_BLOCK, n: int | None = None,
                              time: float | None = None) -> int:
        """Enqueue one frame's whole backward pass (gsr_render_backward_scene, include/gsr.h):
        render_backward into ten record-gradient planes, then project_backward from them into the
        scene-array outputs (as project_backward's, ACCUMULATED, at least one).  Inputs, at least
        one: grad_image_ptr 3*W*H float32 and grad_alpha_ptr W*H.  scratch_ptr: 10*n float32 for
        the planes (colour 3, opacity 1, conic 4, centre 2), zeroed by the call and holding the
        frame's record gradients afterwards; None = a workspace of the context.  A frame that
        overflows adds nothing.  Same returns as render()."""
        gi, ga = _dev_ptr(grad_image_ptr), _dev_ptr(grad_alpha_ptr)
        outs = [_dev_ptr(p) for p in (position_ptr, opacity_ptr, scale_ptr, rot_ptr, sh_ptr, temporal_ptr)]
        if not (gi or ga):
            raise ValueError("render_backward_scene: no upstream gradient given")
        if not any(outs):
            raise ValueError("render_backward_scene: no output requested")
        ptr = scene.ptr if isinstance(scene, Scene) else int(scene)
        n = scene.n if n is None else n
        if isinstance(scene, Scene) and layout == LAYOUT_SCENE_BLOCK:
            layout = scene.layout
        if time is not None:
            self.set_time(time)
        t = tiling or TilingInformation(1, 1, H, W)
        sg = SceneGrads(*[p or None for p in outs])
        rc = lib().gsr_render_backward_scene(self.ctx, ptr, layout, n, byref(cam), W, H, t.num_tile_x, t.num_tile_y,
                                             t.width_stride, t.height_stride, k, gi or None, ga or None,
                                             _dev_ptr(scratch_ptr) or None, byref(sg), stream or None)
        if rc not in (_native.GSR_OK, _native.GSR_E_OVERFLOW):
            raise GsrError(rc, "gsr_render_backward_scene")
        return rc

    def _aux_upstream(self, who, grad_image_ptr, grad_alpha_ptr, grad_depth_ptr, grad_feat_ptr, features_ptr, nfeat,
                      feat_out) -> AuxUpstream:
        """The prechecks the three *_aux calls share, and their gsr_aux_upstream."""
        ups = [_dev_ptr(p) for p in (grad_image_ptr, grad_alpha_ptr, grad_depth_ptr, grad_feat_ptr)]
        feats = _dev_ptr(features_ptr)
        if not any(ups):
            raise ValueError(f"{who}: no upstream gradient given")
        if not 0 <= nfeat <= AUX_MAX_FEATURES:
            raise ValueError(f"{who}: nfeat {nfeat} out of range [0, {AUX_MAX_FEATURES}]")
        if nfeat > 0 and not feats:
            raise ValueError(f"{who}: nfeat {nfeat} needs features_ptr")
        if nfeat == 0 and (ups[3] or feat_out):
            raise ValueError(f"{who}: feature gradients given with nfeat 0")
        return AuxUpstream(*[p or None for p in ups], feats or None, nfeat)

    def render_backward_aux(self, scene, cam: Camera, W: int, H: int, grad_image_ptr=None, grad_alpha_ptr=None,
                            grad_depth_ptr=None, grad_feat_ptr=None, features_ptr=None, nfeat: int = 0,
                            color_ptr=None, opacity_ptr=None, conic_ptr=None, center_ptr=None, z_ptr=None,
                            feat_grad_ptr=None, k: float = 3.0, tiling=None, stream: int = 0,
                            layout: int = LAYOUT_SCENE_BLOCK, n: int | None = None, time: float | None = None) -> int:
        """render_backward with render_aux's depth and feature planes (gsr_render_backward_aux,
        include/gsr.h).  Further inputs: grad_depth_ptr W*H (dL/d the un-normalised depth plane),
        grad_feat_ptr nfeat*W*H planar (dL/d the feature planes) and features_ptr, the nfeat arrays
        of n floats render_aux composites.  Further outputs, ACCUMULATED: z_ptr n floats (dL/d -Z)
        and feat_grad_ptr nfeat planes of n (dL/d the feature values).  At least one input and one
        output; an output whose upstream is missing is not touched.  Same returns as render()."""
        outs = [_dev_ptr(p) for p in (color_ptr, opacity_ptr, conic_ptr, center_ptr, z_ptr, feat_grad_ptr)]
        up = self._aux_upstream("render_backward_aux", grad_image_ptr, grad_alpha_ptr, grad_depth_ptr, grad_feat_ptr,
                                features_ptr, nfeat, outs[5])
        if not any(outs):
            raise ValueError("render_backward_aux: no output requested")
        ptr = scene.ptr if isinstance(scene, Scene) else int(scene)
        n = scene.n if n is None else n
        if isinstance(scene, Scene) and layout == LAYOUT_SCENE_BLOCK:
            layout = scene.layout
        if time is not None:
            self.set_time(time)
        t = tiling or TilingInformation(1, 1, H, W)
        rg = RecordGradsAuxOut(*[o or None for o in outs])
        rc = lib().gsr_render_backward_aux(self.ctx, ptr, layout, n, byref(cam), W, H, t.num_tile_x, t.num_tile_y,
                                           t.width_stride, t.height_stride, k, byref(up), byref(rg), stream or None)
        if rc not in (_native.GSR_OK, _native.GSR_E_OVERFLOW):
            raise GsrError(rc, "gsr_render_backward_aux")
        return rc

    def project_backward_aux(self, scene, cam: Camera, W: int, H: int, d_color_ptr=None, d_opacity_ptr=None,
                             d_conic_ptr=None, d_center_ptr=None, d_z_ptr=None, position_ptr=None, opacity_ptr=None,
                             scale_ptr=None, rot_ptr=None, sh_ptr=None, temporal_ptr=None, k: float = 3.0,
                             stream: int = 0, layout: int = LAYOUT_SCENE_BLOCK, n: int | None = None,
                             time: float | None = None) -> int:
        """project_backward with an eleventh upstream entry (gsr_project_backward_aux,
        include/gsr.h): d_z_ptr, n floats, render_backward_aux's z_ptr (dL/d -Z), carried on to the
        position and, in a 4D scene, the temporal arrays.  Everything else as project_backward."""
        ins = [_dev_ptr(p) for p in (d_color_ptr, d_opacity_ptr, d_conic_ptr, d_center_ptr, d_z_ptr)]
        outs = [_dev_ptr(p) for p in (position_ptr, opacity_ptr, scale_ptr, rot_ptr, sh_ptr, temporal_ptr)]
        if not any(ins):
            raise ValueError("project_backward_aux: no upstream gradient given")
        if not any(outs):
            raise ValueError("project_backward_aux: no output requested")
        ptr = scene.ptr if isinstance(scene, Scene) else int(scene)
        n = scene.n if n is None else n
        if isinstance(scene, Scene) and layout == LAYOUT_SCENE_BLOCK:
            layout = scene.layout
        if time is not None:
            self.set_time(time)
        rg = RecordGradsAux(*[p or None for p in ins])
        sg = SceneGrads(*[p or None for p in outs])
        check(lib().gsr_project_backward_aux(self.ctx, ptr, layout, n, byref(cam), W, H, k, byref(rg), byref(sg),
                                             stream or None), "gsr_project_backward_aux")
        return _native.GSR_OK

    def render_backward_scene_aux(self, scene, cam: Camera, W: int, H: int, grad_image_ptr=None, grad_alpha_ptr=None,
                                  grad_depth_ptr=None, grad_feat_ptr=None, features_ptr=None, nfeat: int = 0,
                                  feat_grad_ptr=None, scratch_ptr=None, position_ptr=None, opacity_ptr=None,
                                  scale_ptr=None, rot_ptr=None, sh_ptr=None, temporal_ptr=None, k: float = 3.0,
                                  tiling=None, stream: int = 0, layout: int = LAYOUT_SCENE_BLOCK,
                                  n: int | None = None, time: float | None = None) -> int:
        """render_backward_scene with the depth and feature planes
        (gsr_render_backward_scene_aux, include/gsr.h): render_backward_aux into ELEVEN record
        planes (the ten of render_backward_scene, then z), project_backward_aux from them.
        scratch_ptr: 11*n float32, or None.  feat_grad_ptr: nfeat planes of n, ACCUMULATED, the
        feature gradients (they have no scene array).  Same returns as render()."""
        outs = [_dev_ptr(p) for p in (position_ptr, opacity_ptr, scale_ptr, rot_ptr, sh_ptr, temporal_ptr)]
        fg = _dev_ptr(feat_grad_ptr)
        up = self._aux_upstream("render_backward_scene_aux", grad_image_ptr, grad_alpha_ptr, grad_depth_ptr,
                                grad_feat_ptr, features_ptr, nfeat, fg)
        if not any(outs):
            raise ValueError("render_backward_scene_aux: no output requested")
        ptr = scene.ptr if isinstance(scene, Scene) else int(scene)
        n = scene.n if n is None else n
        if isinstance(scene, Scene) and layout == LAYOUT_SCENE_BLOCK:
            layout = scene.layout
        if time is not None:
            self.set_time(time)
        t = tiling or TilingInformation(1, 1, H, W)
        sg = SceneGrads(*[p or None for p in outs])
        rc = lib().gsr_render_backward_scene_aux(self.ctx, ptr, layout, n, byref(cam), W, H, t.num_tile_x,
                                                 t.num_tile_y, t.width_stride, t.height_stride, k, byref(up),
                                                 fg or None, _dev_ptr(scratch_ptr) or None, byref(sg), stream or None)
        if rc not in (_native.GSR_OK, _native.GSR_E_OVERFLOW):
            raise GsrError(rc, "gsr_render_backward_scene_aux")
        return rc

    def set_frames_in_flight(self, frames: int):
        """Frames render_path runs concurrently (1..8; lanes 1.. own private workspaces)."""
        check(lib().gsr_set_frames_in_flight(self.ctx, int(frames)), "gsr_set_frames_in_flight")

    def frames_in_flight(self) -> int:
        return int(lib().gsr_frames_in_flight(self.ctx))

    def render_path(self, scene, cams, W: int, H: int, out_ptrs, k: float = 3.0, tiling=None, stream: int = 0,
                    layout: int = LAYOUT_SCENE_BLOCK, n: int | None = None, times=None, events=None,
                    join: bool = True, fork: bool = True, wait_events=None, status=None) -> int:
        """Enqueue len(cams) frames (camera cams[i], 4D time times[i]) into the device
        buffers out_ptrs[i] with up to frames_in_flight() of them concurrent
        (gsr_render_path, include/gsr.h).  Stream-ordered on `stream` at entry and exit.
        events (gsr_render_path_ex): per-frame torch.cuda.Event (or None), recorded on
        frame i's lane after its blend; join=False skips the exit join (the caller then
        orders reads and buffer reuse through the events); wait_events[i] (or None): frame
        i's lane waits for it first; fork=False: lanes 1.. do not wait for `stream`.
        status (gsr_render_path_status): per-frame device address (or None) of a uint32
        validity word, 0 when frame i came out complete, else GSR_FRAME_* bits.
        Same returns as render()."""
        ptr = scene.ptr if isinstance(scene, Scene) else int(scene)
        n = scene.n if n is None else n
        if isinstance(scene, Scene) and layout == LAYOUT_SCENE_BLOCK:
            layout = scene.layout
        nf = len(cams)
        if len(out_ptrs) != nf or (times is not None and len(times) != nf):
            raise ValueError("render_path: cams, out_ptrs and times must have the same length")
        cam_arr = (Camera * max(1, nf))(*cams)
        out_arr = (c_void_p * max(1, nf))(*[int(p) for p in out_ptrs])
        t_arr = (c_float * nf)(*[float(t) for t in times]) if times is not None else None
        t = tiling or TilingInformation(1, 1, H, W)
        if events is None and wait_events is None and join and fork and status is None:
            rc = lib().gsr_render_path(self.ctx, ptr, layout, n, cam_arr, t_arr, nf, W, H, t.num_tile_x,
                                       t.num_tile_y, t.width_stride, t.height_stride, k, out_arr, stream or None)
        else:
            if any(x is not None and len(x) != nf for x in (events, wait_events, status)):
                raise ValueError("render_path: events, wait_events and status must have one entry per frame")
            ev_arr = (c_void_p * max(1, nf))(*[_event_handle(e) for e in (events or [None] * nf)])
            wt_arr = (c_void_p * max(1, nf))(*[_event_handle(e, wait=True) for e in (wait_events or [None] * nf)])
            st_arr = (c_void_p * max(1, nf))(*[int(p) if p else None for p in status]) if status else None
            rc = lib().gsr_render_path_status(self.ctx, ptr, layout, n, cam_arr, t_arr, nf, W, H, t.num_tile_x,
                                              t.num_tile_y, t.width_stride, t.height_stride, k, out_arr,
                                              stream or None, ev_arr, wt_arr,
                                              (0 if join else _native.GSR_PATH_NO_JOIN) |
                                              (0 if fork else _native.GSR_PATH_NO_FORK), st_arr)
        if rc not in (_native.GSR_OK, _native.GSR_E_OVERFLOW):
            raise GsrError(rc, "gsr_render_path")
        return rc

    def render_display(self, target: "DisplayTarget", scene, cam: Camera, W: int, H: int, k: float = 3.0,
                       tiling=None, stream: int = 0, layout: int = LAYOUT_SCENE_BLOCK, n: int | None = None,
                       time: float | None = None) -> int:
        """Enqueue one frame straight into a display target (include/gsr_gl.h):
        map, check it holds 3*W*H floats, render, unmap.  Same returns as render()."""
        ptr = scene.ptr if isinstance(scene, Scene) else int(scene)
        n = scene.n if n is None else n
        if isinstance(scene, Scene) and layout == LAYOUT_SCENE_BLOCK:
            layout = scene.layout
        if time is not None:
            self.set_time(time)
        t = tiling or TilingInformation(1, 1, H, W)
        rc = lib().gsr_render_display(self.ctx, target.ptr, ptr, layout, n, byref(cam), W, H, t.num_tile_x,
                                      t.num_tile_y, t.width_stride, t.height_stride, k, stream or None)
        if rc not in (_native.GSR_OK, _native.GSR_E_OVERFLOW):
            raise GsrError(rc, "gsr_render_display")
        return rc

    def set_time(self, t: float):
        check(lib().gsr_set_time(self.ctx, float(t)), "gsr_set_time")

    def preprocess(self, scene, cam: Camera, W: int, H: int, k: float = 3.0, tiling=None, stream: int = 0,
                   layout: int = LAYOUT_SCENE_BLOCK, n: int | None = None, time: float | None = None):
        ptr = scene.ptr if isinstance(scene, Scene) else int(scene)
        n = scene.n if n is None else n
        if isinstance(scene, Scene) and layout == LAYOUT_SCENE_BLOCK:
            layout = scene.layout
        if time is not None:
            self.set_time(time)
        t = tiling or TilingInformation(1, 1, H, W)
        rc = lib().gsr_preprocess(self.ctx, ptr, layout, n, byref(cam), W, H, t.num_tile_x, t.num_tile_y,
                                  t.width_stride, t.height_stride, k, stream or None)
        if rc not in (_native.GSR_OK, _native.GSR_E_OVERFLOW):
            raise GsrError(rc, "gsr_preprocess")

    def sort(self, stream: int = 0):
        check(lib().gsr_sort(self.ctx, stream or None), "gsr_sort")

    def blend(self, out_ptr: int, stream: int = 0):
        check(lib().gsr_blend(self.ctx, out_ptr, stream or None), "gsr_blend")

    def sync(self) -> int:
        rc = lib().gsr_sync(self.ctx)
        if rc not in (_native.GSR_OK, _native.GSR_E_OVERFLOW):
            raise GsrError(rc, "gsr_sync")
        return rc

    def pair_count(self) -> int:
        return int(lib().gsr_pair_count(self.ctx))

    def row_item_count(self) -> int:
        """(tile row, Gaussian) items of the last frame's row pass; -1 on the pair-sort path."""
        return int(lib().gsr_row_item_count(self.ctx))

    def read_splats(self, n: int) -> np.ndarray:
        out = np.zeros(n, dtype=SPLAT_DTYPE)
        check(lib().gsr_read_splats(self.ctx, out.ctypes.data, n), "gsr_read_splats")
        return out

    def read_depth_order(self, n: int) -> np.ndarray:
        out = np.zeros(n, dtype=np.uint64)
        check(lib().gsr_read_depth_order(self.ctx, out.ctypes.data, n), "gsr_read_depth_order")
        return out

    def read_pairs(self) -> np.ndarray:
        cap = max(self.pair_count(), 0)
        out = np.zeros(max(cap, 1), dtype=np.uint64)
        m = lib().gsr_read_pairs(self.ctx, out.ctypes.data, cap)
        if m < 0:
            raise GsrError(int(m), "gsr_read_pairs")
        return out[:m]

    def tile_grid(self):
        tx, ty = c_int(), c_int()
        check(lib().gsr_tile_grid(self.ctx, byref(tx), byref(ty)), "gsr_tile_grid")
        return tx.value, ty.value

    def read_tile_ranges(self) -> np.ndarray:
        tx, ty = self.tile_grid()
        out = np.zeros((tx * ty, 2), dtype=np.uint32)
        check(lib().gsr_read_tile_ranges(self.ctx, out.ctypes.data, tx * ty), "gsr_read_tile_ranges")
        return out

    def set_timing(self, mode: int, stride: int = 1):
        """0 off, 1 blend events, 2 every stage; events on every `stride`-th frame."""
        check(lib().gsr_set_timing_stride(self.ctx, mode, stride), "gsr_set_timing")

    def set_diagnostics(self, on: bool):
        check(lib().gsr_set_diagnostics(self.ctx, int(on)), "gsr_set_diagnostics")

    def blend_records_loaded(self) -> int:
        return int(lib().gsr_blend_records_loaded(self.ctx))

    def blend_counters(self) -> dict:
        v = np.zeros(8, dtype=np.int64)
        check(lib().gsr_blend_counters(self.ctx, v.ctypes.data), "gsr_blend_counters")
        keys = ("records_loaded", "wave_splat_iters", "active_lanes", "taken_lanes", "slow_path_iters",
                "zero_taken_iters", "lane_slots", "no_candidate_pair_iters")
        return dict(zip(keys, (int(x) for x in v)))

    def blend_counters_ex(self) -> dict:
        """blend_counters() plus the fast-exp blend's re-blended blocks and their
        suspect pixels (gsr_blend_counters_ex)."""
        v = np.zeros(16, dtype=np.int64)
        check(lib().gsr_blend_counters_ex(self.ctx, v.ctypes.data, 16), "gsr_blend_counters_ex")
        d = self.blend_counters()
        d["reblended_blocks"], d["suspect_pixels"] = int(v[8]), int(v[9])
        return d

    def take_map(self, W: int, H: int) -> np.ndarray:
        """Per-pixel take map of the last diagnostics frame (gsr_blend_take_map):
        splats composited | (index-mix sum << 32), shape (H, W)."""
        out = np.zeros((H, W), dtype=np.uint64)
        check(lib().gsr_blend_take_map(self.ctx, out.ctypes.data, out.size), "gsr_blend_take_map")
        return out

    def set_blend_variant(self, variant: int):
        check(lib().gsr_set_blend_variant(self.ctx, int(variant)), "gsr_set_blend_variant")

    def set_tuning(self, knob: int, value: int):
        """gsr_set_tuning: 0 blend schedule, 1 tile-sort items/thread, 2 depth-sort items/thread."""
        check(lib().gsr_set_tuning(self.ctx, int(knob), int(value)), "gsr_set_tuning")

    def get_tuning(self, knob: int) -> int:
        """gsr_get_tuning: the knob's current value (the default unless set)."""
        v = ctypes.c_int(0)
        check(lib().gsr_get_tuning(self.ctx, int(knob), ctypes.byref(v)), "gsr_get_tuning")
        return int(v.value)

    def depth_passes(self) -> int:
        """Depth-sort digit passes the last frame ran (trailing identities are skipped)."""
        rc = lib().gsr_depth_passes(self.ctx)
        if rc < 0:
            raise GsrError(rc, "gsr_depth_passes")
        return rc

    def bucket_sizes(self):
        """gsr_bucket_sizes: per-bucket item counts of the last frame when it was
        bucket-sorted (the last bucket: key 0xFFFFFFFF, the culled items), else None."""
        out = np.zeros(MAX_BUCKETS, dtype=np.uint32)
        rc = lib().gsr_bucket_sizes(self.ctx, out.ctypes.data, out.size)
        if rc < 0:
            raise GsrError(rc, "gsr_bucket_sizes")
        return out[:rc] if rc else None

    def blend_stamps(self, n_groups: int) -> np.ndarray:
        """{start, end} s_memrealtime stamps (100 MHz) per blend workgroup of the
        last diagnostics frame rendered with schedule 2 (one per tile) or 3 (one
        per 8x8 block)."""
        out = np.zeros(2 * n_groups, dtype=np.uint64)
        check(lib().gsr_blend_stamps(self.ctx, out.ctypes.data, out.size), "gsr_blend_stamps")
        return out.reshape(n_groups, 2)

    def stage_times(self):
        ms = (ctypes.c_double * NUM_STAGES)()
        frames = c_int64()
        check(lib().gsr_stage_times(self.ctx, ms, byref(frames)), "gsr_stage_times")
        return dict(zip(STAGES, list(ms))), frames.value


def device_available() -> bool:
    return bool(lib().gsr_device_available())


# gsr_set_tuning knobs used by the tests and tools (include/gsr.h lists them all)
TUNE_DEPTH_SORT_ITEMS = 2
TUNE_DEPTH_SORT_GROUPS = 4
TUNE_TILE_BINNING = 7
TUNE_TILE_SPANS = 19
TUNE_RANK_ATOMIC = 20
TUNE_RANK_ATOMIC_ACTIVE = 21
TUNE_BLEND_EXP = 22
TUNE_DEPTH_SPLIT = 23
TUNE_DEPTH_SPLIT_PERMILLE = 24
TUNE_DEPTH_SPLIT_UNSAT = 25
TUNE_DEPTH_SPLIT_STATE = 26
TUNE_DEPTH_BUCKETS = 28
TUNE_DEPTH_BUCKETS_OVER = 29
TUNE_BUCKET_ROWS = 30
TUNE_COL_CHUNK = 31
TUNE_FAIL_FRAME = 32
TUNE_DEPTH_BUCKETS_WORK = 33
TUNE_PATH_SHARED_PRE = 34
TUNE_PATH_SHARED_LAUNCHES = 35
MAX_BUCKETS = 4096             # gsr_internal.h kMaxBuckets: the bucket sort's largest bucket count


def rank_order_check() -> tuple[int, int]:
    """gsr_rank_order_check: (lane-operations checked, lanes out of lane order) of the
    device self-check behind the atomic rank path (include/gsr.h)."""
    ops, bad = c_int64(0), c_int64(0)
    check(lib().gsr_rank_order_check(byref(ops), byref(bad)), "gsr_rank_order_check")
    return int(ops.value), int(bad.value)


def math_probe(xy: np.ndarray) -> np.ndarray:
    """Evaluate the gsr_detmath functions on the GPU (see include/gsr.h)."""
    xy = np.ascontiguousarray(xy, dtype=np.float32).reshape(-1, 2)
    out = np.zeros((xy.shape[0], 9), dtype=np.float32)
    check(lib().gsr_math_probe(xy.ctypes.data, xy.shape[0], out.ctypes.data), "gsr_math_probe")
    return out


def exp_probe(x_lo: float, x_hi: float, x_big: float) -> tuple[int, int, float, float]:
    """gsr_exp_probe: (monotonicity violations of gsr_blend_expf, packed-loop exp
    mismatches, max relative fast-exp error, the same over x >= x_big) over every float
    in [x_lo, x_hi), on the GPU."""
    v, pk, ea, eb = c_int64(0), c_int64(0), ctypes.c_float(0), ctypes.c_float(0)
    check(lib().gsr_exp_probe2(x_lo, x_hi, x_big, byref(v), byref(pk), byref(ea), byref(eb)), "gsr_exp_probe2")
    return int(v.value), int(pk.value), float(ea.value), float(eb.value)


def alpha_cut_probe(op: np.ndarray) -> np.ndarray:
    """gsr_alpha_take_min_x evaluated on the GPU for each opacity."""
    op = np.ascontiguousarray(op, dtype=np.float32).ravel()
    out = np.zeros_like(op)
    check(lib().gsr_alpha_cut_probe(op.ctypes.data, op.size, out.ctypes.data), "gsr_alpha_cut_probe")
    return out
