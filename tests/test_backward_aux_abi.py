"""The C ABI of gsr_render_backward_aux, gsr_project_backward_aux and
gsr_render_backward_scene_aux on a CPU-only host: the symbols, the layouts of the three new
structs against the ctypes structs, every argument error (returned before any device work), the
Python wrappers' argument checks, and the existing structs' sizes."""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT
from test_abi import exported_symbols

STRUCTS = {
    "gsr_aux_upstream": ("AuxUpstream", ["d_grad_image", "d_grad_alpha", "d_grad_depth", "d_grad_feat", "d_features",
                                         "nfeat"]),
    "gsr_record_grads_aux_out": ("RecordGradsAuxOut", ["d_color", "d_opacity", "d_conic", "d_center", "d_z", "d_feat"]),
    "gsr_record_grads_aux": ("RecordGradsAux", ["d_color", "d_opacity", "d_conic", "d_center", "d_z"]),
}
SYMBOLS = ("gsr_render_backward_aux", "gsr_project_backward_aux", "gsr_render_backward_scene_aux")
# the structs the new entry points sit beside: their sizes are part of the ABI and do not move
EXISTING = {"gsr_backward_targets": ("BackwardTargets", 48), "gsr_record_grads": ("RecordGrads", 32),
            "gsr_scene_grads": ("SceneGrads", 48), "gsr_aux_targets": ("AuxTargets", 40)}
LAYOUT_BLOCK, LAYOUT_AOS, LAYOUT_4D, LAYOUT_SH3 = 0, 1, 2, 3


def c_layout(tmp_path, cname, fields):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gsr.h"\nint main(void) {\n'
                   f'  printf("%zu", sizeof({cname}));\n' +
                   "".join(f'  printf(" %zu", offsetof({cname}, {f}));\n' for f in fields) +
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    return [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]


def test_symbols_exported_and_declared(gsr):
    from gaussianrenderer_amd import _native
    hdr = " ".join(open(os.path.join(ROOT, "include", "gsr.h")).read().replace("*", " ").split())
    for name in SYMBOLS:
        assert name in exported_symbols(_native.LIB_PATH)
        assert name in {n for n, _, _ in _native.SIGNATURES}
        assert f"int {name}(gsr_context ctx" in hdr
        assert hasattr(gsr.Renderer, name[4:])
    for pyname, _ in STRUCTS.values():
        assert pyname in gsr.__all__
    assert "D = depth / alpha" in hdr and "d_grad_depth = g / alpha" in hdr     # the expected-depth recipe


@pytest.mark.parametrize("cname", sorted(STRUCTS))
def test_struct_layout_matches_header(gsr, tmp_path, cname):
    """sizeof / offsetof of the struct as a C compiler sees include/gsr.h."""
    from gaussianrenderer_amd import _native
    pyname, fields = STRUCTS[cname]
    T = getattr(_native, pyname)
    assert [f for f, _ in T._fields_] == fields
    assert c_layout(tmp_path, cname, fields) == [ctypes.sizeof(T)] + [getattr(T, f).offset for f in fields]


@pytest.mark.parametrize("cname", sorted(EXISTING))
def test_existing_struct_sizes_unchanged(gsr, tmp_path, cname):
    from gaussianrenderer_amd import _native
    pyname, size = EXISTING[cname]
    assert c_layout(tmp_path, cname, []) == [size] == [ctypes.sizeof(getattr(_native, pyname))]


def test_render_backward_aux_argument_errors_need_no_device(gsr):
    from gaussianrenderer_amd._native import GSR_E_ARG, AuxUpstream as U, RecordGradsAuxOut as O
    L = gsr.lib()
    cam = gsr.make_camera()
    ctx = L.gsr_create()
    buf = (ctypes.c_float * 64)()   # a host address: the calls below must never touch it
    p = ctypes.addressof(buf)
    ref = lambda s: ctypes.byref(s) if s is not None else None  # noqa: E731

    def call(c, up, out, W=4, n=0, nx=1, camera=cam):
        return L.gsr_render_backward_aux(c, None, 0, n, ctypes.byref(camera) if camera is not None else None, W, 4,
                                         nx, 1, 4, 4, 3.0, ref(up), ref(out), None)

    full_up, full_out = U(p, p, p, p, p, 3), O(p, p, p, p, p, p)
    try:
        assert call(None, full_up, full_out) == GSR_E_ARG                          # no context
        assert call(ctx, None, full_out) == GSR_E_ARG                              # no upstream struct
        assert call(ctx, full_up, None) == GSR_E_ARG                               # no outputs struct
        assert call(ctx, U(None, None, None, None, p, 2), full_out) == GSR_E_ARG   # all four gradients NULL
        assert b"upstream" in L.gsr_last_error()
        assert call(ctx, full_up, O()) == GSR_E_ARG                                # every output NULL
        assert b"no output" in L.gsr_last_error()
        for nfeat in (-1, 9):                                                      # nfeat out of range
            assert call(ctx, U(p, p, p, p, p, nfeat), full_out) == GSR_E_ARG
            assert b"nfeat" in L.gsr_last_error()
        assert call(ctx, U(p, p, p, p, None, 2), full_out) == GSR_E_ARG            # nfeat > 0 without d_features
        assert b"d_features" in L.gsr_last_error()
        assert call(ctx, U(p, p, p, p, None, 0), O(p, p, p, p, p, None)) == GSR_E_ARG      # d_grad_feat, nfeat 0
        assert call(ctx, U(p, p, p, None, None, 0), full_out) == GSR_E_ARG                 # d_feat, nfeat 0
        # the frame arguments gsr_render refuses, with and without the aux channels
        for up, out in ((full_up, full_out), (U(p, None, None, None, None, 0), O(p, None, None, None, None, None)),
                        (U(None, None, p, None, None, 0), O(None, None, None, None, p, None))):
            assert call(ctx, up, out, W=0) == GSR_E_ARG
            assert call(ctx, up, out, n=5) == GSR_E_ARG                            # null scene
            assert call(ctx, up, out, nx=0) == GSR_E_ARG                           # bad tiling
            assert call(ctx, up, out, camera=None) == GSR_E_ARG
        assert not any(buf)
    finally:
        L.gsr_destroy(ctx)


def test_project_backward_aux_argument_errors_need_no_device(gsr):
    from gaussianrenderer_amd._native import GSR_E_ARG, RecordGradsAux as R, SceneGrads as S
    L = gsr.lib()
    cam = gsr.make_camera()
    ctx = L.gsr_create()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    ref = lambda s: ctypes.byref(s) if s is not None else None  # noqa: E731

    def call(c, rg, sg, layout=LAYOUT_BLOCK, W=4, n=0, camera=cam):
        return L.gsr_project_backward_aux(c, None, layout, n, ctypes.byref(camera) if camera is not None else None,
                                          W, 4, 3.0, ref(rg), ref(sg), None)

    full_in, z_only, out5 = R(p, p, p, p, p), R(None, None, None, None, p), S(p, p, p, p, p, None)
    try:
        assert call(None, full_in, out5) == GSR_E_ARG                              # no context
        assert call(ctx, None, out5) == GSR_E_ARG                                  # no inputs struct
        assert call(ctx, full_in, None) == GSR_E_ARG                               # no outputs struct
        assert call(ctx, R(), out5) == GSR_E_ARG                                   # all FIVE inputs NULL
        assert b"upstream" in L.gsr_last_error()
        assert call(ctx, z_only, S()) == GSR_E_ARG                                 # every output NULL
        assert b"no output" in L.gsr_last_error()
        assert call(ctx, z_only, out5, layout=LAYOUT_AOS) == GSR_E_ARG
        assert b"AOS" in L.gsr_last_error()
        for layout in (LAYOUT_BLOCK, LAYOUT_SH3):                                  # d_temporal needs a 4D block
            assert call(ctx, z_only, S(p, p, p, p, p, p), layout=layout) == GSR_E_ARG
            assert b"d_temporal" in L.gsr_last_error()
        for rg in (full_in, z_only):
            assert call(ctx, rg, out5, W=0) == GSR_E_ARG
            assert call(ctx, rg, out5, n=5) == GSR_E_ARG                           # null scene
            assert call(ctx, rg, out5, n=-1) == GSR_E_ARG
            assert call(ctx, rg, out5, layout=7) == GSR_E_ARG
            assert call(ctx, rg, out5, camera=None) == GSR_E_ARG
            # d_z alone is an upstream: n = 0 with valid arguments is a no-op that needs no device
            assert call(ctx, rg, out5) == 0
            assert call(ctx, rg, S(p, p, p, p, p, p), layout=LAYOUT_4D) == 0
        assert not any(buf)
    finally:
        L.gsr_destroy(ctx)


def test_render_backward_scene_aux_argument_errors_need_no_device(gsr):
    from gaussianrenderer_amd._native import GSR_E_ARG, AuxUpstream as U, SceneGrads as S
    L = gsr.lib()
    cam = gsr.make_camera()
    ctx = L.gsr_create()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    ref = lambda s: ctypes.byref(s) if s is not None else None  # noqa: E731

    def call(c, up, sg, feat=None, layout=LAYOUT_BLOCK, W=4, n=0, scratch=None, nx=1, camera=cam):
        return L.gsr_render_backward_scene_aux(c, None, layout, n, ctypes.byref(camera) if camera is not None else None,
                                               W, 4, nx, 1, 4, 4, 3.0, ref(up), feat, scratch, ref(sg), None)

    full_up, depth_up, out5 = U(p, p, p, p, p, 3), U(None, None, p, None, None, 0), S(p, p, p, p, p, None)
    try:
        assert call(None, full_up, out5) == GSR_E_ARG                              # no context
        assert call(ctx, None, out5) == GSR_E_ARG                                  # no upstream struct
        assert call(ctx, U(None, None, None, None, p, 2), out5) == GSR_E_ARG       # all four gradients NULL
        assert b"upstream" in L.gsr_last_error()
        assert call(ctx, full_up, None) == GSR_E_ARG                               # no outputs struct
        assert call(ctx, depth_up, S()) == GSR_E_ARG                               # every output NULL
        assert b"no output" in L.gsr_last_error()
        assert call(ctx, U(p, p, p, p, p, 9), out5, feat=p) == GSR_E_ARG           # nfeat out of range
        assert call(ctx, U(p, p, p, p, None, 2), out5) == GSR_E_ARG                # nfeat > 0 without d_features
        assert call(ctx, depth_up, out5, feat=p) == GSR_E_ARG                      # d_feat_grad, nfeat 0
        assert call(ctx, U(p, None, None, p, None, 0), out5) == GSR_E_ARG          # d_grad_feat, nfeat 0
        assert call(ctx, depth_up, out5, layout=LAYOUT_AOS) == GSR_E_ARG
        assert call(ctx, depth_up, S(p, p, p, p, p, p)) == GSR_E_ARG               # d_temporal, 3D block
        for scratch in (None, p):
            for up, feat in ((full_up, p), (depth_up, None)):
                for sg, layout in ((out5, LAYOUT_BLOCK), (S(None, None, None, p, None, p), LAYOUT_4D)):
                    kw = dict(feat=feat, layout=layout, scratch=scratch)
                    assert call(ctx, up, sg, W=0, **kw) == GSR_E_ARG
                    assert call(ctx, up, sg, n=5, **kw) == GSR_E_ARG               # null scene
                    assert call(ctx, up, sg, nx=0, **kw) == GSR_E_ARG              # bad tiling
                    assert call(ctx, up, sg, camera=None, **kw) == GSR_E_ARG
        assert not any(buf)
    finally:
        L.gsr_destroy(ctx)


def test_python_wrapper_prechecks(gsr):
    class Tensor:
        def data_ptr(self):
            return 0x1000

    r = gsr.Renderer()
    cam = gsr.make_camera()
    t = Tensor()
    try:
        with pytest.raises(ValueError, match="upstream"):
            r.render_backward_aux(1, cam, 4, 4, z_ptr=t, features_ptr=t, nfeat=2, n=0)
        with pytest.raises(ValueError, match="output"):
            r.render_backward_aux(1, cam, 4, 4, grad_depth_ptr=t, n=0)
        with pytest.raises(ValueError, match="nfeat"):
            r.render_backward_aux(1, cam, 4, 4, grad_depth_ptr=t, z_ptr=t, nfeat=9, features_ptr=t, n=0)
        with pytest.raises(ValueError, match="features_ptr"):
            r.render_backward_aux(1, cam, 4, 4, grad_feat_ptr=t, feat_grad_ptr=t, nfeat=2, n=0)
        with pytest.raises(ValueError, match="nfeat 0"):
            r.render_backward_aux(1, cam, 4, 4, grad_feat_ptr=t, z_ptr=t, n=0)
        with pytest.raises(ValueError, match="nfeat 0"):
            r.render_backward_aux(1, cam, 4, 4, grad_depth_ptr=t, feat_grad_ptr=t, n=0)
        with pytest.raises(ValueError, match="upstream"):
            r.project_backward_aux(1, cam, 4, 4, position_ptr=t, n=0)
        with pytest.raises(ValueError, match="output"):
            r.project_backward_aux(1, cam, 4, 4, d_z_ptr=t, n=0)
        with pytest.raises(ValueError, match="upstream"):
            r.render_backward_scene_aux(1, cam, 4, 4, position_ptr=t, scratch_ptr=t, n=0)
        with pytest.raises(ValueError, match="output"):
            r.render_backward_scene_aux(1, cam, 4, 4, grad_depth_ptr=t, scratch_ptr=t, n=0)
        with pytest.raises(ValueError, match="nfeat 0"):
            r.render_backward_scene_aux(1, cam, 4, 4, grad_depth_ptr=t, feat_grad_ptr=t, position_ptr=t, n=0)
        with pytest.raises(ValueError):
            r.render_backward_scene_aux(1, cam, 4, 4, n=0)
        # existing methods keep their signatures
        with pytest.raises(TypeError):
            r.render_backward(1, cam, 4, 4, grad_depth_ptr=t, color_ptr=t, n=0)
    finally:
        r.close()
