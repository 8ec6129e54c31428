"""gsr_project_backward's and gsr_render_backward_scene's C ABI on a CPU-only host: the
symbols, the layouts of gsr_record_grads and gsr_scene_grads against the ctypes structs, the
argument errors (returned before any device work) and the Python wrappers' argument checks."""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT
from test_abi import exported_symbols

STRUCTS = {
    "gsr_record_grads": ("RecordGrads", ["d_color", "d_opacity", "d_conic", "d_center"]),
    "gsr_scene_grads": ("SceneGrads", ["d_position", "d_opacity", "d_scale", "d_rot", "d_sh", "d_temporal"]),
}
SYMBOLS = ("gsr_project_backward", "gsr_render_backward_scene")
LAYOUT_BLOCK, LAYOUT_AOS, LAYOUT_4D, LAYOUT_SH3 = 0, 1, 2, 3


def test_symbols_exported_and_declared(gsr):
    from gaussianrenderer_amd import _native
    hdr = " ".join(open(os.path.join(ROOT, "include", "gsr.h")).read().replace("*", " ").split())
    for name in SYMBOLS:
        assert name in exported_symbols(_native.LIB_PATH)
        assert name in {n for n, _, _ in _native.SIGNATURES}
        assert f"int {name}(gsr_context ctx" in hdr
    assert "ARE reproducible bit for bit" in hdr
    assert hasattr(gsr.Renderer, "project_backward") and hasattr(gsr.Renderer, "render_backward_scene")
    assert "RecordGrads" in gsr.__all__ and "SceneGrads" in gsr.__all__


@pytest.mark.parametrize("cname", sorted(STRUCTS))
def test_struct_layout_matches_header(gsr, tmp_path, cname):
    """sizeof / offsetof of the struct as a C compiler sees include/gsr.h."""
    from gaussianrenderer_amd import _native
    pyname, fields = STRUCTS[cname]
    T = getattr(_native, pyname)
    assert [f for f, _ in T._fields_] == fields
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gsr.h"\nint main(void) {\n'
                   f'  printf("%zu", sizeof({cname}));\n' +
                   "".join(f'  printf(" %zu", offsetof({cname}, {f}));\n' for f in fields) +
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(T)] + [getattr(T, f).offset for f in fields]


def test_project_backward_argument_errors_need_no_device(gsr):
    from gaussianrenderer_amd._native import GSR_E_ARG, RecordGrads as R, SceneGrads as S
    L = gsr.lib()
    cam = gsr.make_camera()
    ctx = L.gsr_create()
    buf = (ctypes.c_float * 64)()   # a host address: the calls below must never touch it
    p = ctypes.addressof(buf)
    ref = lambda s: ctypes.byref(s) if s is not None else None  # noqa: E731

    def call(c, rg, sg, layout=LAYOUT_BLOCK, W=4, n=0, scene=None, camera=cam):
        return L.gsr_project_backward(c, scene, layout, n, ctypes.byref(camera) if camera is not None else None,
                                      W, 4, 3.0, ref(rg), ref(sg), None)

    full_in, out5 = R(p, p, p, p), S(p, p, p, p, p, None)
    try:
        assert call(None, full_in, out5) == GSR_E_ARG                              # no context
        assert call(ctx, None, out5) == GSR_E_ARG                                  # no inputs struct
        assert call(ctx, full_in, None) == GSR_E_ARG                               # no outputs struct
        assert call(ctx, R(), out5) == GSR_E_ARG                                   # every input NULL
        assert b"upstream" in L.gsr_last_error()
        assert call(ctx, full_in, S()) == GSR_E_ARG                                # every output NULL
        assert b"no output" in L.gsr_last_error()
        assert call(ctx, full_in, out5, layout=LAYOUT_AOS) == GSR_E_ARG            # no AoS gradient planes
        assert b"AOS" in L.gsr_last_error()
        for layout in (LAYOUT_BLOCK, LAYOUT_SH3):                                  # d_temporal needs a 4D block
            assert call(ctx, full_in, S(p, p, p, p, p, p), layout=layout) == GSR_E_ARG
            assert b"d_temporal" in L.gsr_last_error()
        # the frame arguments gsr_render refuses, still without a device
        for rg, sg in ((full_in, out5), (R(None, p, None, None), S(None, None, None, None, p, None)),
                       (R(p, None, None, None), S(p, None, None, None, None, None))):
            assert call(ctx, rg, sg, W=0) == GSR_E_ARG
            assert call(ctx, rg, sg, n=5) == GSR_E_ARG                             # null scene
            assert call(ctx, rg, sg, n=-1) == GSR_E_ARG
            assert call(ctx, rg, sg, layout=7) == GSR_E_ARG
            assert call(ctx, rg, sg, camera=None) == GSR_E_ARG
        assert call(ctx, full_in, S(p, p, p, p, p, p), layout=LAYOUT_4D, W=0) == GSR_E_ARG
        # n = 0 with valid arguments is a no-op that needs no device either
        assert call(ctx, full_in, out5) == 0
        assert call(ctx, full_in, S(p, p, p, p, p, p), layout=LAYOUT_4D) == 0
        assert not any(buf)
    finally:
        L.gsr_destroy(ctx)


def test_render_backward_scene_argument_errors_need_no_device(gsr):
    from gaussianrenderer_amd._native import GSR_E_ARG, SceneGrads as S
    L = gsr.lib()
    cam = gsr.make_camera()
    ctx = L.gsr_create()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)

    def call(c, gi, ga, sg, layout=LAYOUT_BLOCK, W=4, n=0, scratch=None, nx=1, camera=cam):
        return L.gsr_render_backward_scene(c, None, layout, n, ctypes.byref(camera) if camera is not None else None,
                                           W, 4, nx, 1, 4, 4, 3.0, gi, ga, scratch,
                                           ctypes.byref(sg) if sg is not None else None, None)

    out5 = S(p, p, p, p, p, None)
    try:
        assert call(None, p, p, out5) == GSR_E_ARG                                 # no context
        assert call(ctx, None, None, out5) == GSR_E_ARG                            # no upstream gradient
        assert b"upstream" in L.gsr_last_error()
        assert call(ctx, p, p, None) == GSR_E_ARG                                  # no outputs struct
        assert call(ctx, p, None, S()) == GSR_E_ARG                                # every output NULL
        assert b"no output" in L.gsr_last_error()
        assert call(ctx, p, p, out5, layout=LAYOUT_AOS) == GSR_E_ARG
        assert call(ctx, None, p, S(p, p, p, p, p, p)) == GSR_E_ARG                # d_temporal, 3D block
        assert call(ctx, None, p, S(p, p, p, p, p, p), layout=LAYOUT_SH3) == GSR_E_ARG
        for scratch in (None, p):
            for sg, layout in ((out5, LAYOUT_BLOCK), (S(None, None, None, p, None, p), LAYOUT_4D)):
                assert call(ctx, p, p, sg, layout=layout, W=0, scratch=scratch) == GSR_E_ARG
                assert call(ctx, p, p, sg, layout=layout, n=5, scratch=scratch) == GSR_E_ARG      # null scene
                assert call(ctx, p, p, sg, layout=layout, nx=0, scratch=scratch) == GSR_E_ARG     # bad tiling
                assert call(ctx, p, p, sg, layout=layout, camera=None, scratch=scratch) == GSR_E_ARG
        assert not any(buf)
    finally:
        L.gsr_destroy(ctx)


def test_python_wrapper_prechecks(gsr):
    class Tensor:
        def data_ptr(self):
            return 0x1000

    r = gsr.Renderer()
    cam = gsr.make_camera()
    try:
        with pytest.raises(ValueError, match="upstream"):
            r.project_backward(1, cam, 4, 4, position_ptr=Tensor(), n=0)
        with pytest.raises(ValueError, match="upstream"):
            r.project_backward(1, cam, 4, 4, d_color_ptr=0, d_conic_ptr=None, sh_ptr=0x2000, n=0)
        with pytest.raises(ValueError, match="output"):
            r.project_backward(1, cam, 4, 4, d_color_ptr=Tensor(), d_center_ptr=0x2000, n=0)
        with pytest.raises(ValueError, match="output"):
            r.project_backward(1, cam, 4, 4, d_opacity_ptr=Tensor(), rot_ptr=0, temporal_ptr=None, n=0)
        with pytest.raises(ValueError):
            r.project_backward(1, cam, 4, 4, n=0)
        with pytest.raises(ValueError, match="upstream"):
            r.render_backward_scene(1, cam, 4, 4, position_ptr=Tensor(), scratch_ptr=Tensor(), n=0)
        with pytest.raises(ValueError, match="output"):
            r.render_backward_scene(1, cam, 4, 4, grad_image_ptr=Tensor(), scratch_ptr=Tensor(), n=0)
        with pytest.raises(ValueError, match="output"):
            r.render_backward_scene(1, cam, 4, 4, grad_alpha_ptr=0x2000, scale_ptr=0, n=0)
        with pytest.raises(ValueError):
            r.render_backward_scene(1, cam, 4, 4, n=0)
    finally:
        r.close()
