"""gsr_render_aux's C ABI on a CPU-only host: the symbol, the layout of gsr_aux_targets
against the ctypes struct, the argument errors (returned before any device work) and the
Python wrapper's argument checks."""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT
from test_abi import exported_symbols


def test_symbol_and_constant(gsr):
    from gaussianrenderer_amd import _native
    assert "gsr_render_aux" in exported_symbols(_native.LIB_PATH)
    assert "gsr_render_aux" in {name for name, _, _ in _native.SIGNATURES}
    assert gsr.AUX_MAX_FEATURES == _native.AUX_MAX_FEATURES == 8
    hdr = open(os.path.join(ROOT, "include", "gsr.h")).read()
    assert "#define GSR_AUX_MAX_FEATURES 8" in hdr
    assert hasattr(gsr.Renderer, "render_aux")


def test_struct_layout_matches_header(gsr, tmp_path):
    """sizeof / offsetof of gsr_aux_targets as a C compiler sees include/gsr.h."""
    from gaussianrenderer_amd._native import AuxTargets
    fields = [f for f, _ in AuxTargets._fields_]
    assert fields == ["d_alpha", "d_depth", "d_features", "nfeat", "d_feat_out"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gsr.h"\nint main(void) {\n'
                   '  printf("%zu", sizeof(gsr_aux_targets));\n' +
                   "".join(f'  printf(" %zu", offsetof(gsr_aux_targets, {f}));\n' for f in fields) +
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(AuxTargets)] + [getattr(AuxTargets, f).offset for f in fields]


def test_argument_errors_need_no_device(gsr):
    from gaussianrenderer_amd._native import AuxTargets, GSR_E_ARG
    L = gsr.lib()
    cam = gsr.make_camera()
    ctx = L.gsr_create()
    buf = (ctypes.c_float * 16)()   # a host address: the calls below must never touch it
    p = ctypes.addressof(buf)

    def call(out, aux):
        return L.gsr_render_aux(ctx, None, 0, 0, ctypes.byref(cam), 4, 4, 1, 1, 4, 4, 3.0, out,
                                ctypes.byref(aux) if aux is not None else None, None)

    try:
        assert call(None, AuxTargets(None, None, None, 0, None)) == GSR_E_ARG          # every output NULL
        assert b"no output" in L.gsr_last_error()
        assert call(p, None) == GSR_E_ARG                                              # no aux struct
        for nfeat in (-1, 9, 1 << 20):
            assert call(p, AuxTargets(p, p, p, nfeat, p)) == GSR_E_ARG                 # nfeat out of range
            assert b"nfeat" in L.gsr_last_error()
        assert call(p, AuxTargets(p, p, None, 2, p)) == GSR_E_ARG                      # features missing
        assert call(p, AuxTargets(p, p, p, 2, None)) == GSR_E_ARG                      # feature output missing
        assert call(None, AuxTargets(None, None, p, 8, None)) == GSR_E_ARG
        assert L.gsr_render_aux(None, None, 0, 0, ctypes.byref(cam), 4, 4, 1, 1, 4, 4, 3.0, p,
                                ctypes.byref(AuxTargets(p, None, None, 0, None)), None) == GSR_E_ARG
        # frame arguments are checked like gsr_render's, still without a device
        assert L.gsr_render_aux(ctx, None, 0, 0, ctypes.byref(cam), 0, 4, 1, 1, 4, 4, 3.0, p,
                                ctypes.byref(AuxTargets(p, None, None, 0, None)), None) == GSR_E_ARG
        assert L.gsr_render_aux(ctx, None, 0, 5, ctypes.byref(cam), 4, 4, 1, 1, 4, 4, 3.0, p,
                                ctypes.byref(AuxTargets(p, None, None, 0, None)), None) == GSR_E_ARG   # null scene
    finally:
        L.gsr_destroy(ctx)


def test_python_wrapper_rejects_inconsistent_arguments(gsr):
    r = gsr.Renderer()
    cam = gsr.make_camera()
    try:
        with pytest.raises((ValueError, gsr.GsrError)):
            r.render_aux(1, cam, 4, 4, n=0)                                            # no output
        with pytest.raises((ValueError, gsr.GsrError)):
            r.render_aux(1, cam, 4, 4, out_ptr=8, nfeat=9, features_ptr=8, feat_out_ptr=8, n=0)
        with pytest.raises((ValueError, gsr.GsrError)):
            r.render_aux(1, cam, 4, 4, out_ptr=8, nfeat=-1, n=0)
        with pytest.raises((ValueError, gsr.GsrError)):
            r.render_aux(1, cam, 4, 4, out_ptr=8, nfeat=2, feat_out_ptr=8, n=0)        # no features
        with pytest.raises((ValueError, gsr.GsrError)):
            r.render_aux(1, cam, 4, 4, out_ptr=8, nfeat=2, features_ptr=8, n=0)        # no feature output
        with pytest.raises((ValueError, gsr.GsrError)):
            r.render_aux(1, cam, 4, 4, out_ptr=8, features_ptr=8, n=0)                 # features, nfeat = 0
    finally:
        r.close()
