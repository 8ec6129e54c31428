"""gsr_render_backward's C ABI on a CPU-only host: the symbol, the layout of
gsr_backward_targets against the ctypes struct, the argument errors (returned before any
device work) and the Python wrapper's argument checks."""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT
from test_abi import exported_symbols

FIELDS = ["d_grad_image", "d_grad_alpha", "d_color", "d_opacity", "d_conic", "d_center"]


def test_symbol_exported_and_declared(gsr):
    from gaussianrenderer_amd import _native
    assert "gsr_render_backward" in exported_symbols(_native.LIB_PATH)
    assert "gsr_render_backward" in {name for name, _, _ in _native.SIGNATURES}
    hdr = open(os.path.join(ROOT, "include", "gsr.h")).read()
    assert "int gsr_render_backward(gsr_context* ctx" in hdr
    assert "NOT reproducible bit for bit" in " ".join(hdr.replace("*", " ").split())
    assert hasattr(gsr.Renderer, "render_backward")
    assert "BackwardTargets" in gsr.__all__


def test_struct_layout_matches_header(gsr, tmp_path):
    """sizeof / offsetof of gsr_backward_targets as a C compiler sees include/gsr.h."""
    from gaussianrenderer_amd._native import BackwardTargets
    assert [f for f, _ in BackwardTargets._fields_] == FIELDS
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gsr.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(gsr_backward_targets));\n' +
                   "".join(f'  printf(" %zu", offsetof(gsr_backward_targets, {f}));\n' for f in FIELDS) +
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(BackwardTargets)] + [getattr(BackwardTargets, f).offset for f in FIELDS]


def test_argument_errors_need_no_device(gsr):
    from gaussianrenderer_amd._native import BackwardTargets as T, GSR_E_ARG
    L = gsr.lib()
    cam = gsr.make_camera()
    ctx = L.gsr_create()
    buf = (ctypes.c_float * 64)()   # a host address: the calls below must never touch it
    p = ctypes.addressof(buf)

    def call(c, bw, W=4, n=0):
        return L.gsr_render_backward(c, None, 0, n, ctypes.byref(cam), W, 4, 1, 1, 4, 4, 3.0,
                                     ctypes.byref(bw) if bw is not None else None, None)

    try:
        assert call(ctx, None) == GSR_E_ARG                                        # no targets struct
        assert call(ctx, T(None, None, p, p, p, p)) == GSR_E_ARG                   # no upstream gradient
        assert b"upstream" in L.gsr_last_error()
        assert call(ctx, T(p, p, None, None, None, None)) == GSR_E_ARG             # every output NULL
        assert b"no output" in L.gsr_last_error()
        assert call(ctx, T()) == GSR_E_ARG
        assert call(None, T(p, p, p, p, p, p)) == GSR_E_ARG                        # no context
        # frame arguments are checked like gsr_render's, still without a device
        for one in (T(p, p, p, p, p, p), T(p, None, p, None, None, None), T(None, p, None, None, None, p)):
            assert call(ctx, one, W=0) == GSR_E_ARG
            assert call(ctx, one, n=5) == GSR_E_ARG                                # null scene
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
            r.render_backward(1, cam, 4, 4, color_ptr=Tensor(), n=0)
        with pytest.raises(ValueError, match="output"):
            r.render_backward(1, cam, 4, 4, grad_image_ptr=Tensor(), grad_alpha_ptr=0x2000, n=0)
        with pytest.raises(ValueError, match="output"):
            r.render_backward(1, cam, 4, 4, grad_alpha_ptr=Tensor(), color_ptr=0, opacity_ptr=None, n=0)
        with pytest.raises(ValueError):
            r.render_backward(1, cam, 4, 4, n=0)
    finally:
        r.close()
