"""gsr_render_contrib's C ABI on a CPU-only host: the symbol, the fixed-point constant, the
layout of gsr_contrib_targets against the ctypes struct, the argument errors (returned
before any device work) and the Python wrapper's argument check."""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT
from test_abi import exported_symbols


def test_symbol_and_constant(gsr):
    from gaussianrenderer_amd import _native
    assert "gsr_render_contrib" in exported_symbols(_native.LIB_PATH)
    assert "gsr_render_contrib" in {name for name, _, _ in _native.SIGNATURES}
    assert gsr.CONTRIB_WEIGHT_ONE == _native.CONTRIB_WEIGHT_ONE == 1 << 24
    hdr = open(os.path.join(ROOT, "include", "gsr.h")).read()
    assert "#define GSR_CONTRIB_WEIGHT_ONE 16777216u" in hdr
    assert hasattr(gsr.Renderer, "render_contrib")
    assert "CONTRIB_WEIGHT_ONE" in gsr.__all__ and "ContribTargets" in gsr.__all__


def test_struct_layout_matches_header(gsr, tmp_path):
    """sizeof / offsetof of gsr_contrib_targets, and the constant, as a C compiler sees include/gsr.h."""
    from gaussianrenderer_amd._native import CONTRIB_WEIGHT_ONE, ContribTargets
    fields = [f for f, _ in ContribTargets._fields_]
    assert fields == ["d_count", "d_weight", "d_max", "d_id"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gsr.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(gsr_contrib_targets));\n' +
                   "".join(f'  printf(" %zu", offsetof(gsr_contrib_targets, {f}));\n' for f in fields) +
                   '  printf(" %u", GSR_CONTRIB_WEIGHT_ONE);\n'
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == ([ctypes.sizeof(ContribTargets)] + [getattr(ContribTargets, f).offset for f in fields] +
                   [CONTRIB_WEIGHT_ONE])


def test_argument_errors_need_no_device(gsr):
    from gaussianrenderer_amd._native import ContribTargets, GSR_E_ARG
    L = gsr.lib()
    cam = gsr.make_camera()
    ctx = L.gsr_create()
    buf = (ctypes.c_uint64 * 16)()   # a host address: the calls below must never touch it
    p = ctypes.addressof(buf)

    def call(c, out, W=4, n=0):
        return L.gsr_render_contrib(c, None, 0, n, ctypes.byref(cam), W, 4, 1, 1, 4, 4, 3.0,
                                    ctypes.byref(out) if out is not None else None, None)

    try:
        assert call(ctx, ContribTargets(None, None, None, None)) == GSR_E_ARG     # every output NULL
        assert b"no output" in L.gsr_last_error()
        assert call(ctx, None) == GSR_E_ARG                                       # no targets struct
        assert call(None, ContribTargets(p, p, p, p)) == GSR_E_ARG                # no context
        # frame arguments are checked like gsr_render's, still without a device
        for one in (ContribTargets(p, p, p, p), ContribTargets(p, None, None, None),
                    ContribTargets(None, None, None, p)):
            assert call(ctx, one, W=0) == GSR_E_ARG
            assert call(ctx, one, n=5) == GSR_E_ARG                               # null scene
        assert not any(buf)
    finally:
        L.gsr_destroy(ctx)


def test_python_wrapper_rejects_no_output(gsr):
    r = gsr.Renderer()
    cam = gsr.make_camera()
    try:
        with pytest.raises(ValueError):
            r.render_contrib(1, cam, 4, 4, n=0)
        with pytest.raises(ValueError):
            r.render_contrib(1, cam, 4, 4, count_ptr=0, weight_ptr=None, max_ptr=0, id_ptr=None, n=0)
    finally:
        r.close()
