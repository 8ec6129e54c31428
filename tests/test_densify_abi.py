"""The scene-densification C ABI (gsr_densify_accumulate, gsr_scene_densify, gsr_densify_normals,
gsr_logf_probe, gsr_densify_gather_planes, gsr_scene_reset_opacity) on a CPU-only host: the
symbols, the struct layouts, the argument errors (returned before any device work: the "device"
pointers below are host buffers that must never be touched), n == 0, and the Python wrappers'
argument checks."""
import ctypes
import os
import re

import pytest

from conftest import ROOT
from test_abi import exported_symbols

NAMES = ("gsr_densify_accumulate", "gsr_scene_densify", "gsr_densify_normals", "gsr_logf_probe",
         "gsr_densify_gather_planes", "gsr_scene_reset_opacity")
INT32_MAX = 2 ** 31 - 1
INF, NAN = float("inf"), float("nan")


def test_symbols_and_signatures(gsr):
    from gaussianrenderer_amd import _native
    syms = exported_symbols(_native.LIB_PATH)
    sigs = {name for name, _, _ in _native.SIGNATURES}
    for name in NAMES:
        assert name in syms and name in sigs, name
    assert hasattr(gsr.Scene, "densify") and hasattr(gsr.Scene, "reset_opacity")
    assert "densify_accumulate" in gsr.__all__ and "densify_gather_planes" in gsr.__all__


def test_struct_layouts_match_the_header(gsr):
    """gsr_densify_config: five floats, padding to 8, the 64-bit seed, the flags, padding to 8;
    gsr_densify_report: five int64.  The field lists are read from include/gsr.h."""
    from gaussianrenderer_amd import _native
    C, R = _native.DensifyConfig, _native.DensifyReport
    assert ctypes.sizeof(C) == 40 and C.seed.offset == 24 and C.flags.offset == 32 and C.split_shrink.offset == 16
    assert ctypes.sizeof(R) == 40
    src = open(os.path.join(ROOT, "include", "gsr.h")).read()
    body = re.search(r"typedef struct gsr_densify_config \{(.*?)\} gsr_densify_config;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(t, n) for t, n in re.findall(r"\b(float|uint64_t|int)\s+(\w+)\s*;", body)]
    ctype = {"float": ctypes.c_float, "uint64_t": ctypes.c_uint64, "int": ctypes.c_int}
    assert [(n, ctype[t]) for t, n in fields] == list(C._fields_)
    rep = re.search(r"typedef struct gsr_densify_report \{\s*int64_t ([^;]*);", src).group(1)
    assert [s.strip() for s in rep.split(",")] == [n for n, _ in R._fields_]
    assert all(t is ctypes.c_int64 for _, t in R._fields_)
    assert _native.DENSIFY_CHUNK == int(re.search(r"constexpr int kDensifyChunk = (\d+);", open(os.path.join(
        ROOT, "gaussianrenderer_amd", "csrc", "gsr_internal.h")).read()).group(1))


def good_config(_native, **kw):
    v = dict(grad_threshold=0.0002, scale_split=0.05, min_opacity=0.005, prune_scale_max=INF, split_shrink=1.6,
             seed=1, flags=0)
    v.update(kw)
    return _native.DensifyConfig(*[v[n] for n, _ in _native.DensifyConfig._fields_])


def test_argument_errors_need_no_device(gsr):
    from gaussianrenderer_amd import _native
    E = _native.GSR_E_ARG
    L = gsr.lib()
    buf = (ctypes.c_uint64 * 128)()   # a host address: the calls below must never touch it
    p = ctypes.addressof(buf)

    def err(name):
        msg = L.gsr_last_error()
        assert name in msg, msg
        return msg

    # gsr_densify_accumulate(d_center, n, W, H, d_grad_accum, d_seen, d_bad, stream)
    for args in ((None, 8, 4, 4, p, p, None, None), (p, 8, 4, 4, None, p, None, None), (p, 8, 4, 4, p, None, None, None),
                 (p, -1, 4, 4, p, p, None, None), (p, INT32_MAX + 1, 4, 4, p, p, None, None),
                 (p, 8, 0, 4, p, p, None, None), (p, 8, 4, -2, p, p, None, None),
                 (p + 2, 8, 4, 4, p, p, None, None), (p, 8, 4, 4, p, p, p + 1, None)):
        assert L.gsr_densify_accumulate(*args) == E, args
        err(b"gsr_densify_accumulate")

    # gsr_scene_densify(d_scene, narrays, n, d_grad_accum, d_seen, cfg, d_src, d_kind, report, stream)
    rep = _native.DensifyReport(-7, -7, -7, -7, -7)
    ok = good_config(_native)

    def densify(scene=p, narrays=38, n=8, accum=p + 256, seen=p + 512, cfg=ok, src=None, kind=None, report=rep):
        return L.gsr_scene_densify(scene, narrays, n, accum, seen, ctypes.byref(cfg) if cfg is not None else None,
                                   src, kind, ctypes.byref(report) if report is not None else None, None)

    # the cases gsr_scene_select refuses, n > INT32_MAX / 2, and the null pointers
    for kw in (dict(scene=None), dict(narrays=37), dict(narrays=0), dict(n=-1), dict(n=INT32_MAX + 1),
               dict(n=INT32_MAX // 2 + 1), dict(n=INT32_MAX), dict(cfg=None), dict(report=None), dict(accum=None),
               dict(seen=None)):
        assert densify(**kw) is None, kw
        err(b"gsr_scene")
    # the configuration
    bad = [dict(grad_threshold=NAN), dict(scale_split=NAN), dict(min_opacity=NAN), dict(prune_scale_max=NAN),
           dict(split_shrink=NAN), dict(grad_threshold=-1e-9), dict(scale_split=-0.5), dict(min_opacity=-0.1),
           dict(min_opacity=1.5), dict(prune_scale_max=0.0), dict(prune_scale_max=-1.0), dict(split_shrink=1.0),
           dict(split_shrink=0.5), dict(split_shrink=INF), dict(split_shrink=-INF), dict(flags=1), dict(flags=-1)]
    for kw in bad:
        assert densify(cfg=good_config(_native, **kw)) is None, kw
        err(b"gsr_scene_densify")
    assert [getattr(rep, n) for n, _ in rep._fields_] == [-7] * 5

    # gsr_densify_gather_planes(d_dst, dst_stride, d_src_planes, src_stride, nplanes, n, d_src, d_kind, m, d_bad, stream)
    def gp(dst=p, ds=8, src=p + 256, ss=8, nplanes=2, n=8, idx=p + 128, kind=p + 192, mm=8, bad=None):
        return L.gsr_densify_gather_planes(dst, ds, src, ss, nplanes, n, idx, kind, mm, bad, None)

    for kw in (dict(dst=None), dict(src=None), dict(idx=None), dict(kind=None), dict(nplanes=0), dict(nplanes=-3),
               dict(n=-1), dict(mm=-1), dict(ss=7), dict(ds=7), dict(mm=INT32_MAX + 1, ds=INT32_MAX + 1),
               dict(n=INT32_MAX + 1, ss=INT32_MAX + 1), dict(n=0, ss=0, mm=1), dict(dst=p + 2), dict(idx=p + 129)):
        assert gp(**kw) == E, kw
        err(b"gsr_densify_gather_planes")

    # gsr_scene_reset_opacity(d_scene, layout, n, cap, d_m_opacity, d_v_opacity, stream)
    for args in ((None, 0, 8, 0.01, None, None, None), (p, 1, 8, 0.01, None, None, None),
                 (p, 7, 8, 0.01, None, None, None), (p, 0, -1, 0.01, None, None, None),
                 (p, 0, INT32_MAX + 1, 0.01, None, None, None), (p, 0, 8, 0.0, None, None, None),
                 (p, 0, 8, 1.0, None, None, None), (p, 0, 8, 5e-7, None, None, None), (p, 0, 8, NAN, None, None, None),
                 (p, 0, 8, -0.5, None, None, None), (p + 2, 0, 8, 0.01, None, None, None),
                 (p, 0, 8, 0.01, p + 1, None, None), (p, 0, 8, 0.01, None, p + 3, None)):
        assert L.gsr_scene_reset_opacity(*args) == E, args
        err(b"gsr_scene_reset_opacity")
    assert not any(buf)


def test_nothing_to_do_needs_no_device(gsr):
    """n == 0 (m == 0) of the stream-ordered calls is GSR_OK without device work; the densify of
    an empty scene reads its header, so it is a GPU test (tests/test_gpu_densify.py)."""
    L = gsr.lib()
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.addressof(buf)
    assert L.gsr_densify_accumulate(None, 0, 4, 4, None, None, None, None) == 0
    gsr.densify_accumulate(None, 0, 4, 4, None, None)
    assert L.gsr_scene_reset_opacity(None, 0, 0, 0.01, None, None, None) == 0
    assert L.gsr_scene_reset_opacity(p, 2, 0, 0.999999, p, p, None) == 0
    assert L.gsr_densify_gather_planes(p, 0, p + 64, 8, 3, 8, p + 128, p + 192, 0, None, None) == 0
    assert not any(buf)


def test_python_wrappers_reject_missing_pointers(gsr):
    s = gsr.Scene(0x1000, 8, owned=False)   # never dereferenced: the wrappers raise first
    with pytest.raises(ValueError):
        s.densify(None, 0x2000, scale_split=0.05)
    with pytest.raises(ValueError):
        s.densify(0x2000, 0, scale_split=0.05)
    with pytest.raises(ValueError):
        gsr.densify_accumulate(None, 8, 4, 4, 0x2000, 0x3000)
    with pytest.raises(ValueError):
        gsr.densify_accumulate(0x1000, 8, 4, 4, 0x2000, None)
    with pytest.raises(ValueError):
        gsr.densify_gather_planes(0x1000, 8, 0x2000, 8, 1, 8, None, 0x3000, 8)
    with pytest.raises(ValueError):
        gsr.densify_gather_planes(0x1000, 8, 0x2000, 8, 1, 8, 0x3000, None, 8)
    with pytest.raises(ValueError):
        gsr.densify_gather_planes(None, 8, 0x2000, 8, 1, 8, 0x3000, 0x4000, 8)
    with pytest.raises(ValueError):
        gsr.Scene(0, 8, owned=False).reset_opacity(0.01)
    # an argument error of the library surfaces as GsrError with its message
    with pytest.raises(gsr.GsrError, match="split_shrink"):
        s.densify(0x2000, 0x3000, scale_split=0.05, split_shrink=1.0)
    with pytest.raises(gsr.GsrError, match="cap"):
        s.reset_opacity(2.0)
