"""Every argument error of the context-free scene API (gsr_scene.cpp): what each call returns
and the exact text gsr_last_error then holds, out of one table.  Rows with two bad arguments at
once pin the order of the checks; rows whose text names gsr_scene_bytes or the PLY reader pin
which callee reports; the n == 0 (m == 0) rows are the successes that need no device.  Host code
only: every row returns before any device work, and the "device" pointers are addresses inside
one host buffer that must stay untouched.

Left out: messages that carry a source file and line (a failed HIP call), every row that would
reach the device (a good gsr_scene_upload, gsr_scene_copy, gsr_scene_download of nothing, ...:
the GPU tests compare those), gsr_densify_normals (no argument error) and
loadGaussianCudaFromPly (C++ linkage, one line over gsr_load_ply_device; tests/test_abi.py pins
its symbol)."""
import ctypes

import pytest

INT32_MAX = 2 ** 31 - 1
INF, NAN = float("inf"), float("nan")
E = -1                                # GSR_E_ARG (include/gsr.h)
NOFILE = b"/nonexistent/gsr_scene_api_errors.ply"
W, H = 8, 4                           # gsr_image_loss's image


class P:
    """An address inside the host buffer: its base + off."""

    def __init__(self, off):
        self.off = off


class S:
    """A struct of _native passed by reference; a field may be a P."""

    def __init__(self, ctype, **fields):
        self.ctype, self.fields = ctype, fields


class N:
    """A scratch size asked of the library when the row runs (see sizes()), plus delta."""

    def __init__(self, key, delta=0):
        self.key, self.delta = key, delta


M_OUT = object()      # gsr_mask_indices / gsr_scene_select: a fresh int64 holding -7
REPORT = object()     # gsr_scene_densify: a fresh gsr_densify_report holding -7 five times
OUT_N = object()      # the loaders: a fresh int holding -7


def grads(off, **over):
    """Five groups' planes at distinct addresses from off on; over: a field -> another value."""
    f = dict(d_position=P(off), d_opacity=P(off + 256), d_scale=P(off + 512), d_rot=P(off + 768), d_sh=P(off + 1024),
             d_temporal=None)
    f.update(over)
    return S("SceneGrads", **f)


def adam(**over):
    f = dict(lr_position=1e-3, lr_opacity=1e-2, lr_scale=1e-3, lr_rot=1e-3, lr_sh_dc=1e-3, lr_sh_rest=1e-4,
             lr_tcenter=0.0, lr_tscale=0.0, lr_motion=0.0, beta1=0.9, beta2=0.999, eps=1e-15, step=1, flags=0)
    f.update(over)
    return S("AdamConfig", **f)


def dens(**over):
    f = dict(grad_threshold=0.0002, scale_split=0.05, min_opacity=0.005, prune_scale_max=INF, split_shrink=1.6,
             seed=1, flags=0)
    f.update(over)
    return S("DensifyConfig", **f)


def init(**over):
    f = dict(opacity=0.1, min_dist2=1e-7, scale_mul=1.0, scale_max=INF, t_center=0.0, t_scale=1.0, flags=0)
    f.update(over)
    return S("InitConfig", **f)


def loss(**over):
    f = dict(w_l1=0.8, w_l2=0.0, w_dssim=0.2, grad_scale=1.0, flags=0)
    f.update(over)
    return S("LossConfig", **f)


T_GRADS = dict(g=grads(2048, d_temporal=P(4096)), m=grads(8192, d_temporal=P(12288)),
               v=grads(16384, d_temporal=P(20480)))

# call: its arguments in order, each with a value that passes every check
DEFAULTS = {
    "gsr_scene_upload_ex": dict(host=P(0), narrays=38, n=8),
    "gsr_scene_upload": dict(host=P(0), n=8),
    "gsr_scene_bytes": dict(narrays=38, n=8),
    "gsr_scene_copy": dict(dst=P(0), scene=P(16384), narrays=38, n=8, stream=None),
    "gsr_mask_indices": dict(keep=P(0), n=8, idx=P(64), m_out=M_OUT, stream=None),
    "gsr_gather_planes": dict(dst=P(0), ds=8, src=P(256), ss=8, nplanes=2, eb=4, n=8, idx=P(128), m=8, bad=None,
                              stream=None),
    "gsr_scene_gather": dict(scene=P(0), narrays=38, n=8, idx=P(16384), m=4, bad=None, stream=None),
    "gsr_scene_select": dict(scene=P(0), narrays=38, n=8, keep=P(16384), m_out=M_OUT, idx=None, stream=None),
    "gsr_scene_adam_step": dict(scene=P(0), layout=0, n=8, g=grads(2048), m=grads(8192), v=grads(16384), c=adam(),
                                bad=None, stream=None),
    "gsr_densify_accumulate": dict(center=P(0), n=8, W=4, H=4, accum=P(256), seen=P(512), bad=None, stream=None),
    "gsr_scene_densify": dict(scene=P(0), narrays=38, n=8, accum=P(16384), seen=P(16640), c=dens(), src=None,
                              kind=None, report=REPORT, stream=None),
    "gsr_logf_probe": dict(x=P(0), n=8, out=P(256)),
    "gsr_densify_gather_planes": dict(dst=P(0), ds=8, src=P(256), ss=8, nplanes=2, n=8, idx=P(128), kind=P(192), m=8,
                                      bad=None, stream=None),
    "gsr_scene_reset_opacity": dict(scene=P(0), layout=0, n=8, cap=0.01, m_op=None, v_op=None, stream=None),
    "gsr_points_knn_scratch_bytes": dict(n=8),
    "gsr_points_knn_dist2": dict(xyz=P(0), ps=3, cs=1, n=8, out=P(512), bad=None, scratch=P(1024), nbytes=N("knn"),
                                 stream=None),
    "gsr_scene_from_points": dict(xyz=P(0), ps=3, cs=1, rgb=P(256), rps=3, rcs=1, n=8, narrays=38, c=init(), out=None,
                                  bad=None, stream=None),
    "gsr_image_loss_scratch_bytes": dict(W=W, H=H, want_grad=1),
    "gsr_image_loss": dict(x=P(0), y=P(1024), W=W, H=H, c=loss(), g=P(2048), l=P(3072), s=P(4096), nbytes=N("grad"),
                           stream=None),
    "gsr_scene_free": dict(d=None),
    "gsr_scene_download": dict(d=P(0), host=P(16384), n=8),
    "gsr_load_ply_device_ex": dict(path=NOFILE, out_n=OUT_N, flags=0, out_narrays=None),
    "gsr_load_ply_device": dict(path=NOFILE, out_n=OUT_N),
}

BYTES = "gsr_scene_bytes: bad argument"
UPLOAD = "gsr_scene_upload: bad argument"
ADAM = "gsr_scene_adam_step: "
LR = ADAM + "a learning rate is negative or not finite"
DENS = "gsr_scene_densify: "
DENS_NAN = DENS + "a NaN field in the configuration"
DGP = "gsr_densify_gather_planes: "
RESET = "gsr_scene_reset_opacity: "
KNN = "gsr_points_knn_dist2: "
INIT = "gsr_scene_from_points: "
INIT_NAN = INIT + "a NaN field in the configuration"
LOSS = "gsr_image_loss: "
WEIGHT = LOSS + "a weight is negative or not finite"
BIG = INT32_MAX + 1
OPEN = "Failed to open file: " + NOFILE.decode()

# (call, arguments other than DEFAULTS', what it returns, the text of gsr_last_error; None:
# a success, which leaves the text alone)
ONE_AT_A_TIME = [
    ("gsr_scene_upload_ex", dict(n=-1), None, UPLOAD),
    ("gsr_scene_upload_ex", dict(n=BIG), None, UPLOAD),
    ("gsr_scene_upload_ex", dict(host=None), None, UPLOAD),
    ("gsr_scene_upload_ex", dict(narrays=37), None, UPLOAD),
    ("gsr_scene_upload_ex", dict(narrays=0), None, UPLOAD),
    ("gsr_scene_upload_ex", dict(narrays=60), None, UPLOAD),
    ("gsr_scene_upload", dict(n=-1), None, UPLOAD),
    ("gsr_scene_upload", dict(n=BIG), None, UPLOAD),
    ("gsr_scene_upload", dict(host=None), None, UPLOAD),

    ("gsr_scene_bytes", dict(n=-1), E, BYTES),
    ("gsr_scene_bytes", dict(n=BIG), E, BYTES),
    ("gsr_scene_bytes", dict(narrays=37), E, BYTES),
    ("gsr_scene_bytes", dict(narrays=0), E, BYTES),
    ("gsr_scene_bytes", dict(narrays=50), E, BYTES),
    ("gsr_scene_bytes", dict(n=0), 256, None),
    ("gsr_scene_bytes", dict(narrays=49, n=0), 256, None),
    ("gsr_scene_bytes", dict(narrays=59, n=0), 256, None),
    ("gsr_scene_bytes", dict(), 256 + 4 * 38 * 64, None),
    ("gsr_scene_bytes", dict(narrays=49, n=65), 256 + 4 * 49 * 128, None),
    ("gsr_scene_bytes", dict(narrays=59, n=INT32_MAX), 256 + 4 * 59 * 2 ** 31, None),

    ("gsr_scene_copy", dict(narrays=37), E, BYTES),
    ("gsr_scene_copy", dict(n=-1), E, BYTES),
    ("gsr_scene_copy", dict(n=BIG), E, BYTES),
    ("gsr_scene_copy", dict(dst=None), E, "gsr_scene_copy: null pointer"),
    ("gsr_scene_copy", dict(scene=None), E, "gsr_scene_copy: null pointer"),

    ("gsr_mask_indices", dict(m_out=None), E, "gsr_mask_indices: null m_out"),
    ("gsr_mask_indices", dict(n=-1), E, "gsr_mask_indices: n = -1 out of range"),
    ("gsr_mask_indices", dict(n=BIG), E, "gsr_mask_indices: n = 2147483648 out of range"),
    ("gsr_mask_indices", dict(keep=None), E, "gsr_mask_indices: null pointer"),
    ("gsr_mask_indices", dict(idx=None), E, "gsr_mask_indices: null pointer"),
    ("gsr_mask_indices", dict(n=0), 0, None),
    ("gsr_mask_indices", dict(n=0, keep=None, idx=None), 0, None),

    ("gsr_gather_planes", dict(dst=None), E, "gsr_gather_planes: null pointer"),
    ("gsr_gather_planes", dict(src=None), E, "gsr_gather_planes: null pointer"),
    ("gsr_gather_planes", dict(idx=None), E, "gsr_gather_planes: null pointer"),
    ("gsr_gather_planes", dict(eb=0), E, "gsr_gather_planes: elem_bytes = 0, not 4 or 8"),
    ("gsr_gather_planes", dict(eb=2), E, "gsr_gather_planes: elem_bytes = 2, not 4 or 8"),
    ("gsr_gather_planes", dict(eb=16), E, "gsr_gather_planes: elem_bytes = 16, not 4 or 8"),
    ("gsr_gather_planes", dict(eb=-4), E, "gsr_gather_planes: elem_bytes = -4, not 4 or 8"),
    ("gsr_gather_planes", dict(nplanes=0), E, "gsr_gather_planes: nplanes = 0 < 1"),
    ("gsr_gather_planes", dict(nplanes=-3), E, "gsr_gather_planes: nplanes = -3 < 1"),
    ("gsr_gather_planes", dict(n=-1), E, "gsr_gather_planes: n = -1, m = 8 out of range"),
    ("gsr_gather_planes", dict(m=-1), E, "gsr_gather_planes: n = 8, m = -1 out of range"),
    ("gsr_gather_planes", dict(m=BIG, ds=BIG), E, "gsr_gather_planes: n = 8, m = 2147483648 out of range"),
    ("gsr_gather_planes", dict(n=BIG, ss=BIG), E, "gsr_gather_planes: n = 2147483648, m = 8 out of range"),
    ("gsr_gather_planes", dict(n=0, ss=0, m=1), E, "gsr_gather_planes: n = 0, m = 1 out of range"),
    ("gsr_gather_planes", dict(ss=7), E,
     "gsr_gather_planes: stride smaller than its count (src 7 < 8 or dst 8 < 8)"),
    ("gsr_gather_planes", dict(ds=7), E,
     "gsr_gather_planes: stride smaller than its count (src 8 < 8 or dst 7 < 8)"),
    ("gsr_gather_planes", dict(dst=P(2)), E, "gsr_gather_planes: misaligned pointer"),
    ("gsr_gather_planes", dict(src=P(257)), E, "gsr_gather_planes: misaligned pointer"),
    ("gsr_gather_planes", dict(eb=8, dst=P(4)), E, "gsr_gather_planes: misaligned pointer"),
    ("gsr_gather_planes", dict(eb=8, src=P(260)), E, "gsr_gather_planes: misaligned pointer"),
    ("gsr_gather_planes", dict(idx=P(130)), E, "gsr_gather_planes: misaligned pointer"),
    ("gsr_gather_planes", dict(bad=P(513)), E, "gsr_gather_planes: misaligned pointer"),
    ("gsr_gather_planes", dict(m=0, ds=0), 0, None),
    ("gsr_gather_planes", dict(n=0, ss=0, m=0, ds=0, eb=8), 0, None),

    ("gsr_scene_gather", dict(m=-1), None, "gsr_scene_gather: m = -1 out of range (n = 8)"),
    ("gsr_scene_gather", dict(m=BIG), None, "gsr_scene_gather: m = 2147483648 out of range (n = 8)"),
    ("gsr_scene_gather", dict(narrays=49, n=0, m=1), None, "gsr_scene_gather: m = 1 out of range (n = 0)"),
    ("gsr_scene_gather", dict(narrays=37), None, BYTES),
    ("gsr_scene_gather", dict(narrays=0), None, BYTES),
    ("gsr_scene_gather", dict(n=-1), None, BYTES),
    ("gsr_scene_gather", dict(n=BIG), None, BYTES),
    ("gsr_scene_gather", dict(scene=None), None, "gsr_scene_gather: null pointer"),
    ("gsr_scene_gather", dict(idx=None), None, "gsr_scene_gather: null pointer"),

    ("gsr_scene_select", dict(narrays=50), None, BYTES),
    ("gsr_scene_select", dict(narrays=59, n=-2, idx=P(32768)), None, BYTES),
    ("gsr_scene_select", dict(narrays=59, n=BIG, idx=P(32768)), None, BYTES),
    ("gsr_scene_select", dict(scene=None), None, "gsr_scene_select: null pointer"),
    ("gsr_scene_select", dict(keep=None), None, "gsr_scene_select: null pointer"),
    ("gsr_scene_select", dict(m_out=None), None, "gsr_scene_select: null pointer"),

    ("gsr_scene_adam_step", dict(g=None), E, ADAM + "null grads, m, v or cfg"),
    ("gsr_scene_adam_step", dict(m=None), E, ADAM + "null grads, m, v or cfg"),
    ("gsr_scene_adam_step", dict(v=None), E, ADAM + "null grads, m, v or cfg"),
    ("gsr_scene_adam_step", dict(c=None), E, ADAM + "null grads, m, v or cfg"),
    ("gsr_scene_adam_step", dict(layout=1), E, ADAM + "layout 1 is not a scene block"),
    ("gsr_scene_adam_step", dict(layout=4), E, ADAM + "layout 4 is not a scene block"),
    ("gsr_scene_adam_step", dict(layout=-1), E, ADAM + "layout -1 is not a scene block"),
    ("gsr_scene_adam_step", dict(n=-1), E, ADAM + "n = -1 out of range"),
    ("gsr_scene_adam_step", dict(n=BIG), E, ADAM + "n = 2147483648 out of range"),
    ("gsr_scene_adam_step", dict(scene=None), E, ADAM + "null scene"),
    ("gsr_scene_adam_step", dict(c=adam(lr_scale=-1e-3)), E, LR),
    ("gsr_scene_adam_step", dict(c=adam(lr_motion=-1.0)), E, LR),          # of a frozen group
    ("gsr_scene_adam_step", dict(c=adam(lr_position=INF)), E, LR),
    ("gsr_scene_adam_step", dict(c=adam(lr_sh_rest=NAN)), E, LR),
    ("gsr_scene_adam_step", dict(c=adam(beta1=1.0)), E, ADAM + "beta1 = 1, beta2 = 0.999 outside [0, 1)"),
    ("gsr_scene_adam_step", dict(c=adam(beta1=-0.1)), E, ADAM + "beta1 = -0.1, beta2 = 0.999 outside [0, 1)"),
    ("gsr_scene_adam_step", dict(c=adam(beta1=NAN)), E, ADAM + "beta1 = nan, beta2 = 0.999 outside [0, 1)"),
    ("gsr_scene_adam_step", dict(c=adam(beta2=1.0)), E, ADAM + "beta1 = 0.9, beta2 = 1 outside [0, 1)"),
    ("gsr_scene_adam_step", dict(c=adam(beta2=-1e-3)), E, ADAM + "beta1 = 0.9, beta2 = -0.001 outside [0, 1)"),
    ("gsr_scene_adam_step", dict(c=adam(eps=0.0)), E, ADAM + "eps = 0"),
    ("gsr_scene_adam_step", dict(c=adam(eps=-1e-8)), E, ADAM + "eps = -1e-08"),
    ("gsr_scene_adam_step", dict(c=adam(eps=INF)), E, ADAM + "eps = inf"),
    ("gsr_scene_adam_step", dict(c=adam(eps=NAN)), E, ADAM + "eps = nan"),
    ("gsr_scene_adam_step", dict(c=adam(step=0)), E, ADAM + "step = 0 < 1"),
    ("gsr_scene_adam_step", dict(c=adam(step=-5)), E, ADAM + "step = -5 < 1"),
    ("gsr_scene_adam_step", dict(c=adam(flags=4)), E, ADAM + "unknown flag bits 0x4"),
    ("gsr_scene_adam_step", dict(c=adam(flags=3 | 8)), E, ADAM + "unknown flag bits 0xb"),
    ("gsr_scene_adam_step", dict(c=adam(lr_tcenter=1e-3, lr_tscale=1e-3, lr_motion=1e-3), **T_GRADS), E,
     ADAM + "d_temporal needs a 4D scene block"),
    ("gsr_scene_adam_step", dict(layout=3, c=adam(lr_motion=1e-3), **T_GRADS), E,
     ADAM + "d_temporal needs a 4D scene block"),
    ("gsr_scene_adam_step", dict(m=grads(8192, d_scale=None)), E, ADAM + "an active group lacks a moment plane"),
    ("gsr_scene_adam_step", dict(v=grads(16384, d_opacity=None)), E, ADAM + "an active group lacks a moment plane"),
    ("gsr_scene_adam_step", dict(v=grads(16384, d_sh=None), c=adam(lr_sh_dc=0)), E,   # sh_rest alone active
     ADAM + "an active group lacks a moment plane"),
    ("gsr_scene_adam_step", dict(layout=2, g=T_GRADS["g"], c=adam(lr_tscale=1e-3)), E,
     ADAM + "an active group lacks a moment plane"),
    ("gsr_scene_adam_step", dict(g=S("SceneGrads")), E,
     ADAM + "no active group (a gradient pointer with a non-zero lr)"),
    ("gsr_scene_adam_step", dict(c=adam(lr_position=0, lr_opacity=0, lr_scale=0, lr_rot=0, lr_sh_dc=0, lr_sh_rest=0)),
     E, ADAM + "no active group (a gradient pointer with a non-zero lr)"),
    ("gsr_scene_adam_step", dict(g=S("SceneGrads", d_rot=P(2048)), c=adam(lr_rot=0)), E,
     ADAM + "no active group (a gradient pointer with a non-zero lr)"),
    ("gsr_scene_adam_step", dict(scene=P(2)), E, ADAM + "misaligned pointer"),
    ("gsr_scene_adam_step", dict(g=grads(2048, d_rot=P(2048 + 769))), E, ADAM + "misaligned pointer"),
    ("gsr_scene_adam_step", dict(m=grads(8192, d_position=P(8193))), E, ADAM + "misaligned pointer"),
    ("gsr_scene_adam_step", dict(v=grads(16384, d_sh=P(16386))), E, ADAM + "misaligned pointer"),
    ("gsr_scene_adam_step", dict(bad=P(30001)), E, ADAM + "misaligned pointer"),
    # a frozen group needs no moments and its pointer no alignment; a frozen d_temporal may go with a 3D block
    ("gsr_scene_adam_step", dict(n=0), 0, None),
    ("gsr_scene_adam_step", dict(n=0, scene=None, layout=2), 0, None),
    ("gsr_scene_adam_step", dict(n=0, scene=None, layout=3, c=adam(flags=3)), 0, None),
    ("gsr_scene_adam_step", dict(n=0, m=grads(8192, d_rot=None), v=grads(16384, d_rot=None), c=adam(lr_rot=0)), 0,
     None),
    ("gsr_scene_adam_step", dict(n=0, g=grads(2048, d_temporal=P(4096))), 0, None),
    ("gsr_scene_adam_step", dict(n=0, g=grads(2048, d_rot=P(2048 + 769)), c=adam(lr_rot=0)), 0, None),

    ("gsr_densify_accumulate", dict(n=-1), E, "gsr_densify_accumulate: n = -1 out of range"),
    ("gsr_densify_accumulate", dict(n=BIG), E, "gsr_densify_accumulate: n = 2147483648 out of range"),
    ("gsr_densify_accumulate", dict(W=0), E, "gsr_densify_accumulate: 0 x 4 out of range"),
    ("gsr_densify_accumulate", dict(H=-2), E, "gsr_densify_accumulate: 4 x -2 out of range"),
    ("gsr_densify_accumulate", dict(center=None), E, "gsr_densify_accumulate: null pointer"),
    ("gsr_densify_accumulate", dict(accum=None), E, "gsr_densify_accumulate: null pointer"),
    ("gsr_densify_accumulate", dict(seen=None), E, "gsr_densify_accumulate: null pointer"),
    ("gsr_densify_accumulate", dict(center=P(2)), E, "gsr_densify_accumulate: misaligned pointer"),
    ("gsr_densify_accumulate", dict(accum=P(257)), E, "gsr_densify_accumulate: misaligned pointer"),
    ("gsr_densify_accumulate", dict(seen=P(515)), E, "gsr_densify_accumulate: misaligned pointer"),
    ("gsr_densify_accumulate", dict(bad=P(1025)), E, "gsr_densify_accumulate: misaligned pointer"),
    ("gsr_densify_accumulate", dict(n=0), 0, None),
    ("gsr_densify_accumulate", dict(n=0, center=None, accum=None, seen=None), 0, None),

    ("gsr_scene_densify", dict(narrays=37), None, BYTES),
    ("gsr_scene_densify", dict(narrays=0), None, BYTES),
    ("gsr_scene_densify", dict(n=-1), None, BYTES),
    ("gsr_scene_densify", dict(n=BIG), None, BYTES),
    ("gsr_scene_densify", dict(n=INT32_MAX // 2 + 1), None,
     DENS + "n = 1073741824 > INT32_MAX / 2 (the expansion can double it)"),
    ("gsr_scene_densify", dict(n=INT32_MAX), None,
     DENS + "n = 2147483647 > INT32_MAX / 2 (the expansion can double it)"),
    ("gsr_scene_densify", dict(scene=None), None, DENS + "null pointer"),
    ("gsr_scene_densify", dict(c=None), None, DENS + "null pointer"),
    ("gsr_scene_densify", dict(report=None), None, DENS + "null pointer"),
    ("gsr_scene_densify", dict(accum=None), None, DENS + "null pointer"),
    ("gsr_scene_densify", dict(seen=None), None, DENS + "null pointer"),
    ("gsr_scene_densify", dict(c=dens(grad_threshold=NAN)), None, DENS_NAN),
    ("gsr_scene_densify", dict(c=dens(scale_split=NAN)), None, DENS_NAN),
    ("gsr_scene_densify", dict(c=dens(min_opacity=NAN)), None, DENS_NAN),
    ("gsr_scene_densify", dict(c=dens(prune_scale_max=NAN)), None, DENS_NAN),
    ("gsr_scene_densify", dict(c=dens(split_shrink=NAN)), None, DENS_NAN),
    ("gsr_scene_densify", dict(c=dens(grad_threshold=-1e-9)), None,
     DENS + "grad_threshold = -1e-09 or scale_split = 0.05 negative"),
    ("gsr_scene_densify", dict(c=dens(scale_split=-0.5)), None,
     DENS + "grad_threshold = 0.0002 or scale_split = -0.5 negative"),
    ("gsr_scene_densify", dict(c=dens(min_opacity=-0.1)), None, DENS + "min_opacity = -0.1 outside [0, 1]"),
    ("gsr_scene_densify", dict(c=dens(min_opacity=1.5)), None, DENS + "min_opacity = 1.5 outside [0, 1]"),
    ("gsr_scene_densify", dict(c=dens(prune_scale_max=0.0)), None, DENS + "prune_scale_max = 0 <= 0"),
    ("gsr_scene_densify", dict(c=dens(prune_scale_max=-1.0)), None, DENS + "prune_scale_max = -1 <= 0"),
    ("gsr_scene_densify", dict(c=dens(split_shrink=1.0)), None, DENS + "split_shrink = 1 not finite or <= 1"),
    ("gsr_scene_densify", dict(c=dens(split_shrink=0.5)), None, DENS + "split_shrink = 0.5 not finite or <= 1"),
    ("gsr_scene_densify", dict(c=dens(split_shrink=INF)), None, DENS + "split_shrink = inf not finite or <= 1"),
    ("gsr_scene_densify", dict(c=dens(split_shrink=-INF)), None, DENS + "split_shrink = -inf not finite or <= 1"),
    ("gsr_scene_densify", dict(c=dens(flags=1)), None, DENS + "unknown flag bits 0x1"),
    ("gsr_scene_densify", dict(c=dens(flags=-1)), None, DENS + "unknown flag bits 0xffffffff"),
    ("gsr_scene_densify", dict(accum=P(16386)), None, DENS + "misaligned pointer"),
    ("gsr_scene_densify", dict(seen=P(16641)), None, DENS + "misaligned pointer"),
    ("gsr_scene_densify", dict(src=P(32771)), None, DENS + "misaligned pointer"),

    ("gsr_logf_probe", dict(x=None), E, "gsr_logf_probe: bad argument"),
    ("gsr_logf_probe", dict(out=None), E, "gsr_logf_probe: bad argument"),
    ("gsr_logf_probe", dict(n=-1), E, "gsr_logf_probe: bad argument"),
    ("gsr_logf_probe", dict(n=0), 0, None),

    ("gsr_densify_gather_planes", dict(dst=None), E, DGP + "null pointer"),
    ("gsr_densify_gather_planes", dict(src=None), E, DGP + "null pointer"),
    ("gsr_densify_gather_planes", dict(idx=None), E, DGP + "null pointer"),
    ("gsr_densify_gather_planes", dict(kind=None), E, DGP + "null pointer"),
    ("gsr_densify_gather_planes", dict(nplanes=0), E, DGP + "nplanes = 0 < 1"),
    ("gsr_densify_gather_planes", dict(nplanes=-3), E, DGP + "nplanes = -3 < 1"),
    ("gsr_densify_gather_planes", dict(n=-1), E, DGP + "n = -1, m = 8 out of range"),
    ("gsr_densify_gather_planes", dict(m=-1), E, DGP + "n = 8, m = -1 out of range"),
    ("gsr_densify_gather_planes", dict(m=BIG, ds=BIG), E, DGP + "n = 8, m = 2147483648 out of range"),
    ("gsr_densify_gather_planes", dict(n=BIG, ss=BIG), E, DGP + "n = 2147483648, m = 8 out of range"),
    ("gsr_densify_gather_planes", dict(n=0, ss=0, m=1), E, DGP + "n = 0, m = 1 out of range"),
    ("gsr_densify_gather_planes", dict(ss=7), E, DGP + "stride smaller than its count (src 7 < 8 or dst 8 < 8)"),
    ("gsr_densify_gather_planes", dict(ds=7), E, DGP + "stride smaller than its count (src 8 < 8 or dst 7 < 8)"),
    ("gsr_densify_gather_planes", dict(dst=P(2)), E, DGP + "misaligned pointer"),
    ("gsr_densify_gather_planes", dict(src=P(259)), E, DGP + "misaligned pointer"),
    ("gsr_densify_gather_planes", dict(idx=P(129)), E, DGP + "misaligned pointer"),
    ("gsr_densify_gather_planes", dict(bad=P(514)), E, DGP + "misaligned pointer"),
    ("gsr_densify_gather_planes", dict(m=0, ds=0, dst=P(0), src=P(64), nplanes=3), 0, None),
    ("gsr_densify_gather_planes", dict(m=0, kind=P(193)), 0, None),        # d_kind is bytes

    ("gsr_scene_reset_opacity", dict(layout=1), E, RESET + "layout 1 is not a scene block"),
    ("gsr_scene_reset_opacity", dict(layout=7), E, RESET + "layout 7 is not a scene block"),
    ("gsr_scene_reset_opacity", dict(n=-1), E, RESET + "n = -1 out of range"),
    ("gsr_scene_reset_opacity", dict(n=BIG), E, RESET + "n = 2147483648 out of range"),
    ("gsr_scene_reset_opacity", dict(scene=None), E, RESET + "null scene"),
    ("gsr_scene_reset_opacity", dict(cap=0.0), E, RESET + "cap = 0 outside [1e-06, 0.999999]"),
    ("gsr_scene_reset_opacity", dict(cap=1.0), E, RESET + "cap = 1 outside [1e-06, 0.999999]"),
    ("gsr_scene_reset_opacity", dict(cap=5e-7), E, RESET + "cap = 5e-07 outside [1e-06, 0.999999]"),
    ("gsr_scene_reset_opacity", dict(cap=NAN), E, RESET + "cap = nan outside [1e-06, 0.999999]"),
    ("gsr_scene_reset_opacity", dict(cap=-0.5), E, RESET + "cap = -0.5 outside [1e-06, 0.999999]"),
    ("gsr_scene_reset_opacity", dict(scene=P(2)), E, RESET + "misaligned pointer"),
    ("gsr_scene_reset_opacity", dict(m_op=P(257)), E, RESET + "misaligned pointer"),
    ("gsr_scene_reset_opacity", dict(v_op=P(515)), E, RESET + "misaligned pointer"),
    ("gsr_scene_reset_opacity", dict(n=0, scene=None), 0, None),
    ("gsr_scene_reset_opacity", dict(n=0, layout=2, cap=0.999999, m_op=P(256), v_op=P(512)), 0, None),
    ("gsr_scene_reset_opacity", dict(n=0, layout=3, cap=1e-6), 0, None),

    ("gsr_points_knn_scratch_bytes", dict(n=-1), E, "gsr_points_knn_scratch_bytes: n = -1 out of range"),
    ("gsr_points_knn_scratch_bytes", dict(n=BIG), E, "gsr_points_knn_scratch_bytes: n = 2147483648 out of range"),
    ("gsr_points_knn_scratch_bytes", dict(n=0), 0, None),

    ("gsr_points_knn_dist2", dict(n=-1), E, KNN + "n = -1 out of range"),
    ("gsr_points_knn_dist2", dict(n=BIG), E, KNN + "n = 2147483648 out of range"),
    ("gsr_points_knn_dist2", dict(xyz=None), E, KNN + "null d_xyz"),
    ("gsr_points_knn_dist2", dict(ps=0), E, KNN + "point stride < 1 (0, 1)"),
    ("gsr_points_knn_dist2", dict(cs=0), E, KNN + "point stride < 1 (3, 0)"),
    ("gsr_points_knn_dist2", dict(ps=-3), E, KNN + "point stride < 1 (-3, 1)"),
    ("gsr_points_knn_dist2", dict(cs=-1), E, KNN + "point stride < 1 (3, -1)"),
    ("gsr_points_knn_dist2", dict(cs=2 ** 62), E, KNN + "point strides (3, 4611686018427387904) out of range"),
    ("gsr_points_knn_dist2", dict(ps=2 ** 62), E, KNN + "point strides (4611686018427387904, 1) out of range"),
    ("gsr_points_knn_dist2", dict(ps=1, cs=1), E, KNN + "point strides (1, 1) overlap for n = 8"),
    ("gsr_points_knn_dist2", dict(ps=3, cs=3), E, KNN + "point strides (3, 3) overlap for n = 8"),
    ("gsr_points_knn_dist2", dict(ps=2, cs=1), E, KNN + "point strides (2, 1) overlap for n = 8"),
    ("gsr_points_knn_dist2", dict(ps=1, cs=7), E, KNN + "point strides (1, 7) overlap for n = 8"),
    ("gsr_points_knn_dist2", dict(ps=4, cs=2), E, KNN + "point strides (4, 2) overlap for n = 8"),
    ("gsr_points_knn_dist2", dict(ps=2, cs=15), E, KNN + "point strides (2, 15) overlap for n = 8"),
    ("gsr_points_knn_dist2", dict(xyz=P(2)), E, KNN + "misaligned pointer"),
    ("gsr_points_knn_dist2", dict(out=P(513)), E, KNN + "misaligned pointer"),
    ("gsr_points_knn_dist2", dict(bad=P(1)), E, KNN + "misaligned pointer"),
    ("gsr_points_knn_dist2", dict(out=None), E, KNN + "null d_mean2 or d_scratch"),
    ("gsr_points_knn_dist2", dict(scratch=None), E, KNN + "null d_mean2 or d_scratch"),
    ("gsr_points_knn_dist2", dict(scratch=P(1026)), E, KNN + "misaligned pointer"),
    ("gsr_points_knn_dist2", dict(nbytes=N("knn", -1)), E, KNN + "scratch_bytes = {knn-1}, {knn} needed"),
    ("gsr_points_knn_dist2", dict(nbytes=0), E, KNN + "scratch_bytes = 0, {knn} needed"),
    ("gsr_points_knn_dist2", dict(n=0, nbytes=0), 0, None),
    ("gsr_points_knn_dist2", dict(n=0, xyz=None, out=None, scratch=None, nbytes=0), 0, None),
    ("gsr_points_knn_dist2", dict(n=0, ps=1, cs=64), 0, None),

    ("gsr_scene_from_points", dict(n=-1), None, INIT + "n = -1 out of range"),
    ("gsr_scene_from_points", dict(n=BIG), None, INIT + "n = 2147483648 out of range"),
    ("gsr_scene_from_points", dict(xyz=None), None, INIT + "null d_xyz"),
    ("gsr_scene_from_points", dict(ps=0), None, INIT + "point stride < 1 (0, 1)"),
    ("gsr_scene_from_points", dict(cs=-1), None, INIT + "point stride < 1 (3, -1)"),
    ("gsr_scene_from_points", dict(cs=2 ** 62), None, INIT + "point strides (3, 4611686018427387904) out of range"),
    ("gsr_scene_from_points", dict(ps=1, cs=1), None, INIT + "point strides (1, 1) overlap for n = 8"),
    ("gsr_scene_from_points", dict(ps=2, cs=1), None, INIT + "point strides (2, 1) overlap for n = 8"),
    ("gsr_scene_from_points", dict(ps=1, cs=7), None, INIT + "point strides (1, 7) overlap for n = 8"),
    ("gsr_scene_from_points", dict(xyz=P(2)), None, INIT + "misaligned pointer"),
    ("gsr_scene_from_points", dict(out=P(514)), None, INIT + "misaligned pointer"),
    ("gsr_scene_from_points", dict(bad=P(3)), None, INIT + "misaligned pointer"),
    ("gsr_scene_from_points", dict(rps=0), None, INIT + "rgb stride < 1 (0, 1)"),
    ("gsr_scene_from_points", dict(rcs=0), None, INIT + "rgb stride < 1 (3, 0)"),
    ("gsr_scene_from_points", dict(rps=2 ** 62), None, INIT + "rgb strides (4611686018427387904, 1) out of range"),
    ("gsr_scene_from_points", dict(rps=2, rcs=2), None, INIT + "rgb strides (2, 2) overlap for n = 8"),
    ("gsr_scene_from_points", dict(rps=2, rcs=1), None, INIT + "rgb strides (2, 1) overlap for n = 8"),
    ("gsr_scene_from_points", dict(rps=1, rcs=7), None, INIT + "rgb strides (1, 7) overlap for n = 8"),
    ("gsr_scene_from_points", dict(rgb=P(257)), None, INIT + "misaligned pointer"),
    ("gsr_scene_from_points", dict(narrays=37), None, INIT + "narrays = 37"),
    ("gsr_scene_from_points", dict(narrays=0), None, INIT + "narrays = 0"),
    ("gsr_scene_from_points", dict(narrays=60), None, INIT + "narrays = 60"),
    ("gsr_scene_from_points", dict(c=None), None, INIT + "null cfg"),
    ("gsr_scene_from_points", dict(c=init(opacity=NAN)), None, INIT_NAN),
    ("gsr_scene_from_points", dict(c=init(min_dist2=NAN)), None, INIT_NAN),
    ("gsr_scene_from_points", dict(c=init(scale_mul=NAN)), None, INIT_NAN),
    ("gsr_scene_from_points", dict(c=init(scale_max=NAN)), None, INIT_NAN),
    ("gsr_scene_from_points", dict(c=init(t_center=NAN)), None, INIT_NAN),
    ("gsr_scene_from_points", dict(c=init(t_scale=NAN)), None, INIT_NAN),
    ("gsr_scene_from_points", dict(c=init(opacity=0.0)), None, INIT + "opacity = 0 outside [1e-06, 0.999999]"),
    ("gsr_scene_from_points", dict(c=init(opacity=1.0)), None, INIT + "opacity = 1 outside [1e-06, 0.999999]"),
    ("gsr_scene_from_points", dict(c=init(opacity=5e-7)), None, INIT + "opacity = 5e-07 outside [1e-06, 0.999999]"),
    ("gsr_scene_from_points", dict(c=init(opacity=-0.1)), None, INIT + "opacity = -0.1 outside [1e-06, 0.999999]"),
    ("gsr_scene_from_points", dict(c=init(min_dist2=-1e-9)), None, INIT + "min_dist2 = -1e-09 < 0"),
    ("gsr_scene_from_points", dict(c=init(scale_mul=0.0)), None, INIT + "scale_mul = 0 not finite or <= 0"),
    ("gsr_scene_from_points", dict(c=init(scale_mul=-1.0)), None, INIT + "scale_mul = -1 not finite or <= 0"),
    ("gsr_scene_from_points", dict(c=init(scale_mul=INF)), None, INIT + "scale_mul = inf not finite or <= 0"),
    ("gsr_scene_from_points", dict(c=init(scale_max=0.0)), None, INIT + "scale_max = 0 <= 0"),
    ("gsr_scene_from_points", dict(c=init(scale_max=-2.0)), None, INIT + "scale_max = -2 <= 0"),
    ("gsr_scene_from_points", dict(narrays=49, c=init(t_scale=0.0)), None, INIT + "t_scale = 0 <= 0 on a 4D block"),
    ("gsr_scene_from_points", dict(narrays=49, c=init(t_scale=-1.0)), None, INIT + "t_scale = -1 <= 0 on a 4D block"),
    ("gsr_scene_from_points", dict(c=init(flags=1)), None, INIT + "unknown flag bits 0x1"),
    ("gsr_scene_from_points", dict(c=init(flags=-1)), None, INIT + "unknown flag bits 0xffffffff"),

    ("gsr_image_loss_scratch_bytes", dict(W=0), E, "gsr_image_loss_scratch_bytes: 0 x 4 out of range"),
    ("gsr_image_loss_scratch_bytes", dict(H=-1, want_grad=0), E, "gsr_image_loss_scratch_bytes: 8 x -1 out of range"),
    ("gsr_image_loss_scratch_bytes", dict(W=32768, H=21846), E,
     "gsr_image_loss_scratch_bytes: 32768 x 21846 out of range"),
    ("gsr_image_loss_scratch_bytes", dict(W=65536, H=65536), E,
     "gsr_image_loss_scratch_bytes: 65536 x 65536 out of range"),

    ("gsr_image_loss", dict(x=None), E, LOSS + "null image, target or cfg"),
    ("gsr_image_loss", dict(y=None), E, LOSS + "null image, target or cfg"),
    ("gsr_image_loss", dict(c=None), E, LOSS + "null image, target or cfg"),
    ("gsr_image_loss", dict(g=None, l=None), E, LOSS + "neither a gradient nor the loss values asked for"),
    ("gsr_image_loss", dict(W=0), E, LOSS + "0 x 4 out of range"),
    ("gsr_image_loss", dict(W=-8), E, LOSS + "-8 x 4 out of range"),
    ("gsr_image_loss", dict(H=0), E, LOSS + "8 x 0 out of range"),
    ("gsr_image_loss", dict(H=-1), E, LOSS + "8 x -1 out of range"),
    ("gsr_image_loss", dict(W=32768, H=21846, nbytes=2 ** 62), E, LOSS + "32768 x 21846 out of range"),
    ("gsr_image_loss", dict(W=65536, H=65536, nbytes=2 ** 62), E, LOSS + "65536 x 65536 out of range"),
    ("gsr_image_loss", dict(c=loss(w_l1=-0.8)), E, WEIGHT),
    ("gsr_image_loss", dict(c=loss(w_l2=-1e-3)), E, WEIGHT),
    ("gsr_image_loss", dict(c=loss(w_dssim=-0.2)), E, WEIGHT),
    ("gsr_image_loss", dict(c=loss(w_l1=INF)), E, WEIGHT),
    ("gsr_image_loss", dict(c=loss(w_l2=NAN)), E, WEIGHT),
    ("gsr_image_loss", dict(c=loss(w_dssim=NAN)), E, WEIGHT),
    ("gsr_image_loss", dict(c=loss(w_l1=0.0, w_l2=0.0, w_dssim=0.0)), E, LOSS + "every weight is 0"),
    ("gsr_image_loss", dict(c=loss(grad_scale=INF)), E, LOSS + "grad_scale = inf"),
    ("gsr_image_loss", dict(c=loss(grad_scale=NAN)), E, LOSS + "grad_scale = nan"),
    ("gsr_image_loss", dict(c=loss(flags=1)), E, LOSS + "unknown flag bits 0x1"),
    ("gsr_image_loss", dict(c=loss(flags=1 << 30)), E, LOSS + "unknown flag bits 0x40000000"),
    ("gsr_image_loss", dict(s=None), E, LOSS + "null scratch"),
    ("gsr_image_loss", dict(nbytes=N("grad", -1)), E, LOSS + "scratch_bytes = {grad-1}, {grad} needed"),
    ("gsr_image_loss", dict(nbytes=N("value")), E, LOSS + "scratch_bytes = {value}, {grad} needed"),
    ("gsr_image_loss", dict(g=None, nbytes=N("value", -1)), E, LOSS + "scratch_bytes = {value-1}, {value} needed"),
    ("gsr_image_loss", dict(nbytes=0), E, LOSS + "scratch_bytes = 0, {grad} needed"),
    ("gsr_image_loss", dict(nbytes=-1), E, LOSS + "scratch_bytes = -1, {grad} needed"),
    ("gsr_image_loss", dict(x=P(2)), E, LOSS + "misaligned pointer"),
    ("gsr_image_loss", dict(y=P(1025)), E, LOSS + "misaligned pointer"),
    ("gsr_image_loss", dict(g=P(2051)), E, LOSS + "misaligned pointer"),
    ("gsr_image_loss", dict(l=P(3074)), E, LOSS + "misaligned pointer"),
    ("gsr_image_loss", dict(s=P(4097)), E, LOSS + "misaligned pointer"),
    ("gsr_image_loss", dict(g=P(0)), E,
     LOSS + "d_grad_image is d_image or d_target (the gradient launch reads both)"),
    ("gsr_image_loss", dict(g=P(1024)), E,
     LOSS + "d_grad_image is d_image or d_target (the gradient launch reads both)"),

    ("gsr_scene_free", dict(), None, None),

    ("gsr_scene_download", dict(d=None), E, "gsr_scene_download: bad argument"),
    ("gsr_scene_download", dict(host=None), E, "gsr_scene_download: bad argument"),
    ("gsr_scene_download", dict(n=-1), E, "gsr_scene_download: bad argument"),

    # the loaders report what the PLY reader (gsr_ply.cpp) refused; *out_n is left alone
    ("gsr_load_ply_device_ex", dict(), None, OPEN),
    ("gsr_load_ply_device_ex", dict(flags=2, out_n=None), None, OPEN),
    ("gsr_load_ply_device_ex", dict(path=None), None, "gsr_ply_read_host: null argument"),
    ("gsr_load_ply_device", dict(), None, OPEN),
    ("gsr_load_ply_device", dict(path=None), None, "gsr_ply_read_host: null argument"),
]

# two bad arguments at once: the check that comes first reports
TWO_AT_ONCE = [
    ("gsr_scene_upload_ex", dict(n=-1, narrays=0), None, UPLOAD),
    ("gsr_scene_upload", dict(n=BIG, host=None), None, UPLOAD),
    ("gsr_scene_bytes", dict(n=-1, narrays=0), E, BYTES),
    ("gsr_scene_copy", dict(narrays=0, dst=None), E, BYTES),
    ("gsr_scene_copy", dict(n=-1, scene=None), E, BYTES),
    ("gsr_mask_indices", dict(m_out=None, n=-1), E, "gsr_mask_indices: null m_out"),
    ("gsr_mask_indices", dict(n=-1, keep=None), E, "gsr_mask_indices: n = -1 out of range"),
    ("gsr_mask_indices", dict(m_out=None, n=0), E, "gsr_mask_indices: null m_out"),
    ("gsr_gather_planes", dict(dst=None, eb=0), E, "gsr_gather_planes: null pointer"),
    ("gsr_gather_planes", dict(eb=2, nplanes=0), E, "gsr_gather_planes: elem_bytes = 2, not 4 or 8"),
    ("gsr_gather_planes", dict(nplanes=0, n=-1), E, "gsr_gather_planes: nplanes = 0 < 1"),
    ("gsr_gather_planes", dict(m=-1, ss=7), E, "gsr_gather_planes: n = 8, m = -1 out of range"),
    ("gsr_gather_planes", dict(ss=7, dst=P(2)), E,
     "gsr_gather_planes: stride smaller than its count (src 7 < 8 or dst 8 < 8)"),
    ("gsr_gather_planes", dict(ss=7, ds=6), E,
     "gsr_gather_planes: stride smaller than its count (src 7 < 8 or dst 6 < 8)"),
    ("gsr_scene_gather", dict(m=-1, narrays=0), None, "gsr_scene_gather: m = -1 out of range (n = 8)"),
    ("gsr_scene_gather", dict(m=1, n=0, narrays=0), None, "gsr_scene_gather: m = 1 out of range (n = 0)"),
    ("gsr_scene_gather", dict(narrays=0, scene=None), None, BYTES),
    ("gsr_scene_gather", dict(n=-1, idx=None), None, BYTES),
    ("gsr_scene_select", dict(narrays=50, scene=None), None, BYTES),
    ("gsr_scene_select", dict(n=-1, m_out=None, keep=None), None, BYTES),
    ("gsr_scene_adam_step", dict(c=None, layout=1), E, ADAM + "null grads, m, v or cfg"),
    ("gsr_scene_adam_step", dict(layout=1, n=-1), E, ADAM + "layout 1 is not a scene block"),
    ("gsr_scene_adam_step", dict(n=-1, scene=None), E, ADAM + "n = -1 out of range"),
    ("gsr_scene_adam_step", dict(scene=None, c=adam(lr_rot=-1.0)), E, ADAM + "null scene"),
    ("gsr_scene_adam_step", dict(c=adam(lr_rot=NAN, beta1=1.0)), E, LR),
    ("gsr_scene_adam_step", dict(c=adam(beta2=1.0, eps=0.0)), E, ADAM + "beta1 = 0.9, beta2 = 1 outside [0, 1)"),
    ("gsr_scene_adam_step", dict(c=adam(eps=0.0, step=0)), E, ADAM + "eps = 0"),
    ("gsr_scene_adam_step", dict(c=adam(step=0, flags=4)), E, ADAM + "step = 0 < 1"),
    ("gsr_scene_adam_step", dict(c=adam(flags=4, lr_motion=1e-3), **T_GRADS), E, ADAM + "unknown flag bits 0x4"),
    ("gsr_scene_adam_step", dict(g=grads(2048, d_temporal=P(4096)), m=grads(8192, d_scale=None),
                                 c=adam(lr_motion=1e-3)), E, ADAM + "an active group lacks a moment plane"),
    ("gsr_scene_adam_step", dict(g=grads(2048, d_temporal=P(4096)), scene=P(2), c=adam(lr_motion=1e-3)), E,
     ADAM + "d_temporal needs a 4D scene block"),
    ("gsr_scene_adam_step", dict(g=S("SceneGrads"), scene=P(2)), E,
     ADAM + "no active group (a gradient pointer with a non-zero lr)"),
    ("gsr_scene_adam_step", dict(n=0, bad=P(30001)), E, ADAM + "misaligned pointer"),
    ("gsr_densify_accumulate", dict(n=-1, W=0), E, "gsr_densify_accumulate: n = -1 out of range"),
    ("gsr_densify_accumulate", dict(W=0, center=None), E, "gsr_densify_accumulate: 0 x 4 out of range"),
    ("gsr_densify_accumulate", dict(center=None, bad=P(1025)), E, "gsr_densify_accumulate: null pointer"),
    ("gsr_densify_accumulate", dict(n=0, H=0), E, "gsr_densify_accumulate: 4 x 0 out of range"),
    ("gsr_densify_accumulate", dict(n=0, seen=P(514)), E, "gsr_densify_accumulate: misaligned pointer"),
    ("gsr_scene_densify", dict(narrays=0, n=INT32_MAX), None, BYTES),
    ("gsr_scene_densify", dict(n=INT32_MAX, scene=None), None,
     DENS + "n = 2147483647 > INT32_MAX / 2 (the expansion can double it)"),
    ("gsr_scene_densify", dict(c=None, accum=P(16386)), None, DENS + "null pointer"),
    ("gsr_scene_densify", dict(report=None, c=dens(flags=1)), None, DENS + "null pointer"),
    ("gsr_scene_densify", dict(c=dens(split_shrink=NAN, grad_threshold=-1.0)), None, DENS_NAN),
    ("gsr_scene_densify", dict(c=dens(scale_split=-0.5, min_opacity=2.0)), None,
     DENS + "grad_threshold = 0.0002 or scale_split = -0.5 negative"),
    ("gsr_scene_densify", dict(c=dens(min_opacity=2.0, prune_scale_max=0.0)), None,
     DENS + "min_opacity = 2 outside [0, 1]"),
    ("gsr_scene_densify", dict(c=dens(prune_scale_max=0.0, split_shrink=1.0)), None, DENS + "prune_scale_max = 0 <= 0"),
    ("gsr_scene_densify", dict(c=dens(split_shrink=1.0, flags=2)), None, DENS + "split_shrink = 1 not finite or <= 1"),
    ("gsr_scene_densify", dict(c=dens(flags=2), seen=P(16641)), None, DENS + "unknown flag bits 0x2"),
    ("gsr_logf_probe", dict(x=None, n=-1), E, "gsr_logf_probe: bad argument"),
    ("gsr_densify_gather_planes", dict(kind=None, nplanes=0), E, DGP + "null pointer"),
    ("gsr_densify_gather_planes", dict(nplanes=0, m=-1), E, DGP + "nplanes = 0 < 1"),
    ("gsr_densify_gather_planes", dict(n=-1, ds=7), E, DGP + "n = -1, m = 8 out of range"),
    ("gsr_densify_gather_planes", dict(ds=7, idx=P(129)), E,
     DGP + "stride smaller than its count (src 8 < 8 or dst 7 < 8)"),
    ("gsr_scene_reset_opacity", dict(layout=1, n=-1), E, RESET + "layout 1 is not a scene block"),
    ("gsr_scene_reset_opacity", dict(n=-1, scene=None), E, RESET + "n = -1 out of range"),
    ("gsr_scene_reset_opacity", dict(scene=None, cap=0.0), E, RESET + "null scene"),
    ("gsr_scene_reset_opacity", dict(cap=0.0, scene=P(2)), E, RESET + "cap = 0 outside [1e-06, 0.999999]"),
    ("gsr_scene_reset_opacity", dict(n=0, m_op=P(257)), E, RESET + "misaligned pointer"),
    ("gsr_points_knn_dist2", dict(n=-1, xyz=None), E, KNN + "n = -1 out of range"),
    ("gsr_points_knn_dist2", dict(xyz=None, ps=0), E, KNN + "null d_xyz"),
    ("gsr_points_knn_dist2", dict(ps=0, cs=2 ** 62), E, KNN + "point stride < 1 (0, 4611686018427387904)"),
    ("gsr_points_knn_dist2", dict(ps=2 ** 62, cs=2 ** 62), E,
     KNN + "point strides (4611686018427387904, 4611686018427387904) out of range"),
    ("gsr_points_knn_dist2", dict(ps=2, xyz=P(2)), E, KNN + "point strides (2, 1) overlap for n = 8"),
    ("gsr_points_knn_dist2", dict(xyz=P(2), out=None), E, KNN + "misaligned pointer"),
    ("gsr_points_knn_dist2", dict(out=None, scratch=P(1026)), E, KNN + "null d_mean2 or d_scratch"),
    ("gsr_points_knn_dist2", dict(scratch=P(1026), nbytes=0), E, KNN + "misaligned pointer"),
    ("gsr_points_knn_dist2", dict(n=0, ps=3, cs=3), E, KNN + "point strides (3, 3) overlap for n = 0"),
    ("gsr_scene_from_points", dict(n=-1, rps=0), None, INIT + "n = -1 out of range"),
    ("gsr_scene_from_points", dict(xyz=P(2), rps=0), None, INIT + "misaligned pointer"),
    ("gsr_scene_from_points", dict(rps=0, rgb=P(257)), None, INIT + "rgb stride < 1 (0, 1)"),
    ("gsr_scene_from_points", dict(rgb=P(257), narrays=37), None, INIT + "misaligned pointer"),
    ("gsr_scene_from_points", dict(rgb=None, rps=0, rcs=0, narrays=37), None, INIT + "narrays = 37"),   # no d_rgb: its strides are not looked at
    ("gsr_scene_from_points", dict(narrays=37, c=None), None, INIT + "narrays = 37"),
    ("gsr_scene_from_points", dict(c=init(t_scale=NAN, opacity=0.0)), None, INIT_NAN),
    ("gsr_scene_from_points", dict(c=init(opacity=0.0, min_dist2=-1.0)), None,
     INIT + "opacity = 0 outside [1e-06, 0.999999]"),
    ("gsr_scene_from_points", dict(c=init(min_dist2=-1.0, scale_mul=0.0)), None, INIT + "min_dist2 = -1 < 0"),
    ("gsr_scene_from_points", dict(c=init(scale_mul=0.0, scale_max=0.0)), None,
     INIT + "scale_mul = 0 not finite or <= 0"),
    ("gsr_scene_from_points", dict(c=init(scale_max=0.0, flags=1)), None, INIT + "scale_max = 0 <= 0"),
    ("gsr_scene_from_points", dict(narrays=49, c=init(t_scale=0.0, flags=1)), None,
     INIT + "t_scale = 0 <= 0 on a 4D block"),
    ("gsr_scene_from_points", dict(c=init(t_scale=0.0, flags=1)), None, INIT + "unknown flag bits 0x1"),
    ("gsr_scene_from_points", dict(narrays=59, c=init(t_scale=-1.0, flags=4)), None, INIT + "unknown flag bits 0x4"),
    ("gsr_image_loss_scratch_bytes", dict(W=0, H=0), E, "gsr_image_loss_scratch_bytes: 0 x 0 out of range"),
    ("gsr_image_loss", dict(x=None, g=None, l=None), E, LOSS + "null image, target or cfg"),
    ("gsr_image_loss", dict(g=None, l=None, W=0), E, LOSS + "neither a gradient nor the loss values asked for"),
    ("gsr_image_loss", dict(W=0, c=loss(w_l1=-1.0)), E, LOSS + "0 x 4 out of range"),
    ("gsr_image_loss", dict(c=loss(w_l1=0.0, w_l2=0.0, w_dssim=-0.0, grad_scale=NAN)), E, LOSS + "every weight is 0"),
    ("gsr_image_loss", dict(c=loss(w_l2=-1.0, grad_scale=INF)), E, WEIGHT),
    ("gsr_image_loss", dict(c=loss(grad_scale=INF, flags=1)), E, LOSS + "grad_scale = inf"),
    ("gsr_image_loss", dict(c=loss(flags=1), s=None), E, LOSS + "unknown flag bits 0x1"),
    ("gsr_image_loss", dict(s=None, nbytes=0), E, LOSS + "null scratch"),
    ("gsr_image_loss", dict(nbytes=0, x=P(2)), E, LOSS + "scratch_bytes = 0, {grad} needed"),
    ("gsr_image_loss", dict(g=P(1024), l=P(3074)), E, LOSS + "misaligned pointer"),
    ("gsr_scene_download", dict(d=None, n=-1), E, "gsr_scene_download: bad argument"),
    ("gsr_load_ply_device_ex", dict(path=None, out_n=None), None, "gsr_ply_read_host: null argument"),
    ("gsr_load_ply_device", dict(path=None, out_n=None), None, "gsr_ply_read_host: null argument"),
]

TABLE = ONE_AT_A_TIME + TWO_AT_ONCE
NO_ARGUMENT_ERROR = {"gsr_scene_free"}
ONE_ARGUMENT = {"gsr_points_knn_scratch_bytes"}
# every entry point of gsr_scene.cpp with C linkage but gsr_densify_normals (no argument to refuse)
MOVED = {"gsr_scene_upload_ex", "gsr_scene_bytes", "gsr_scene_copy", "gsr_mask_indices", "gsr_gather_planes",
         "gsr_scene_gather", "gsr_scene_select", "gsr_scene_adam_step", "gsr_densify_accumulate",
         "gsr_scene_densify", "gsr_logf_probe", "gsr_densify_gather_planes", "gsr_scene_reset_opacity",
         "gsr_points_knn_scratch_bytes", "gsr_points_knn_dist2", "gsr_scene_from_points",
         "gsr_image_loss_scratch_bytes", "gsr_image_loss", "gsr_scene_upload", "gsr_scene_free",
         "gsr_scene_download", "gsr_load_ply_device_ex", "gsr_load_ply_device"}


def test_the_table_covers_every_entry_point():
    assert set(DEFAULTS) == MOVED
    assert {row[0] for row in TABLE} == MOVED
    refused = {row[0] for row in TABLE if row[3] is not None}
    assert refused == MOVED - NO_ARGUMENT_ERROR
    assert {row[0] for row in TWO_AT_ONCE} == MOVED - NO_ARGUMENT_ERROR - ONE_ARGUMENT
    for call, over, _, _ in TABLE:
        assert set(over) <= set(DEFAULTS[call]), (call, over)


@pytest.fixture(scope="module")
def host(gsr):
    """The host buffer the "device" pointers point into."""
    buf = (ctypes.c_uint64 * 32768)()
    return buf, ctypes.addressof(buf)


@pytest.fixture(scope="module")
def sizes(gsr):
    """The scratch sizes the texts quote, asked of the library."""
    L = gsr.lib()
    s = {"knn": L.gsr_points_knn_scratch_bytes(8), "grad": L.gsr_image_loss_scratch_bytes(W, H, 1),
         "value": L.gsr_image_loss_scratch_bytes(W, H, 0)}
    assert 0 < s["knn"] and 0 < s["value"] < s["grad"] <= 8 * 32768 - 4096
    return s


@pytest.mark.parametrize("row", range(len(TABLE)), ids=lambda i: f"{TABLE[i][0]}-{i}")
def test_row(gsr, host, sizes, row):
    from gaussianrenderer_amd import _native
    call, over, want, text = TABLE[row]
    buf, base = host
    L = gsr.lib()
    keep = []   # what the call's pointers point to

    def resolve(v):
        if isinstance(v, P):
            return base + v.off
        if isinstance(v, N):
            return sizes[v.key] + v.delta
        if isinstance(v, S):
            st = getattr(_native, v.ctype)(**{k: resolve(f) for k, f in v.fields.items()})
            keep.append(st)
            return ctypes.byref(st)
        if v is M_OUT:
            keep.append(ctypes.c_int64(-7))
            return ctypes.byref(keep[-1])
        if v is OUT_N:
            keep.append(ctypes.c_int(-7))
            return ctypes.byref(keep[-1])
        if v is REPORT:
            keep.append(_native.DensifyReport(-7, -7, -7, -7, -7))
            return ctypes.byref(keep[-1])
        return v

    args = dict(DEFAULTS[call])
    args.update(over)
    if text is None:   # a success leaves the text alone: put a known one there
        assert L.gsr_scene_bytes(0, 0) == E and L.gsr_last_error() == BYTES.encode()
    got = getattr(L, call)(*[resolve(v) for v in args.values()])
    assert got == want, (call, over, L.gsr_last_error())
    if text is None:
        assert L.gsr_last_error() == BYTES.encode(), (call, over)
    else:
        quoted = {k + d: v + int(d or 0) for k, v in sizes.items() for d in ("", "-1")}
        for k, v in quoted.items():
            text = text.replace("{" + k + "}", str(v))
        assert L.gsr_last_error().decode() == text, (call, over)
    # outputs: an error leaves them alone; gsr_mask_indices of nothing counts nothing
    for out in keep:
        if isinstance(out, (ctypes.c_int64, ctypes.c_int)):
            assert out.value == (0 if text is None else -7), (call, over)
        elif isinstance(out, _native.DensifyReport):
            assert [getattr(out, n) for n, _ in out._fields_] == [-7] * 5, (call, over)
    assert not any(buf), (call, over)
