"""The scene-initialisation C ABI (gsr_points_knn_scratch_bytes, gsr_points_knn_dist2,
gsr_scene_from_points) on a CPU-only host: the symbols, the struct layout, the argument errors
(returned before any device work: the "device" pointers below are host buffers that must never be
touched), n == 0, the scratch size's monotonicity, and the Python wrappers' argument checks."""
import ctypes
import os
import re

import pytest

from conftest import ROOT
from test_abi import exported_symbols

NAMES = ("gsr_points_knn_scratch_bytes", "gsr_points_knn_dist2", "gsr_scene_from_points")
INT32_MAX = 2 ** 31 - 1
INF, NAN = float("inf"), float("nan")


def test_symbols_and_signatures(gsr):
    from gaussianrenderer_amd import _native
    syms = exported_symbols(_native.LIB_PATH)
    sigs = {name for name, _, _ in _native.SIGNATURES}
    for name in NAMES:
        assert name in syms and name in sigs, name
    assert hasattr(gsr.Scene, "from_points") and hasattr(gsr.Scene, "knn_dist2")
    assert "points_knn_dist2" in gsr.__all__ and "points_knn_scratch_bytes" in gsr.__all__


def test_struct_layout_and_constants_match_the_sources(gsr):
    """gsr_init_config: six floats and the flags, 28 bytes; the field list is read from
    include/gsr.h, the structure's constants from gsr_internal.h."""
    from gaussianrenderer_amd import _native
    C = _native.InitConfig
    assert ctypes.sizeof(C) == 28 and C.flags.offset == 24 and C.t_scale.offset == 20
    src = open(os.path.join(ROOT, "include", "gsr.h")).read()
    body = re.search(r"typedef struct gsr_init_config \{(.*?)\} gsr_init_config;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(float|int)\s+(\w+)\s*;", body)
    ctype = {"float": ctypes.c_float, "int": ctypes.c_int}
    assert [(n, ctype[t]) for t, n in fields] == list(C._fields_)
    internal = open(os.path.join(ROOT, "gaussianrenderer_amd", "csrc", "gsr_internal.h")).read()
    for py, cname in (("KNN_LEAF", "kKnnLeaf"), ("KNN_FAN", "kKnnFan"), ("KNN_BOUNDS_CHUNK", "kKnnBoundsChunk")):
        assert getattr(_native, py) == int(re.search(rf"constexpr int {cname} = (\d+);", internal).group(1))
    assert _native.KNN_SORT_TILE == 256 * 16 and "kSortTile = kSortThreads * 16" in internal
    assert _native.SCENE_HEADER_BYTES == 256


def good_config(_native, **kw):
    v = dict(opacity=0.1, min_dist2=1e-7, scale_mul=1.0, scale_max=INF, t_center=0.0, t_scale=1.0, flags=0)
    v.update(kw)
    return _native.InitConfig(*[v[n] for n, _ in _native.InitConfig._fields_])


def test_argument_errors_need_no_device(gsr):
    from gaussianrenderer_amd import _native
    E = _native.GSR_E_ARG
    L = gsr.lib()
    buf = (ctypes.c_uint64 * 512)()   # a host address: the calls below must never touch it
    p = ctypes.addressof(buf)
    need = L.gsr_points_knn_scratch_bytes(8)
    assert need > 0

    def err(name):
        msg = L.gsr_last_error()
        assert name in msg, msg
        return msg

    # gsr_points_knn_dist2(d_xyz, point_stride, comp_stride, n, d_mean2, d_bad, d_scratch, scratch_bytes, stream)
    def knn(xyz=p, ps=3, cs=1, n=8, out=p + 512, bad=None, scratch=p + 1024, nbytes=need):
        return L.gsr_points_knn_dist2(xyz, ps, cs, n, out, bad, scratch, nbytes, None)

    for kw in (dict(xyz=None), dict(out=None), dict(scratch=None), dict(n=-1), dict(n=INT32_MAX + 1),
               dict(ps=0), dict(cs=0), dict(ps=-3), dict(cs=-1), dict(ps=1, cs=1), dict(ps=3, cs=3),
               dict(ps=2, cs=1), dict(ps=1, cs=7), dict(ps=4, cs=2), dict(ps=2, cs=15),
               dict(nbytes=need - 1), dict(nbytes=0), dict(xyz=p + 2), dict(out=p + 513), dict(bad=p + 1),
               dict(scratch=p + 1026)):
        assert knn(**kw) == E, kw
        err(b"gsr_points_knn_dist2")
    # n == 0: GSR_OK without device work, with or without pointers
    assert L.gsr_points_knn_dist2(None, 3, 1, 0, None, None, None, 0, None) == 0
    assert knn(n=0, nbytes=0) == 0
    assert knn(n=0, ps=1, cs=64) == 0
    gsr.points_knn_dist2(None, 0, None, None, 0)

    # gsr_scene_from_points(d_xyz, ps, cs, d_rgb, rps, rcs, n, narrays, cfg, d_mean2, d_bad, stream)
    ok = good_config(_native)

    def init(xyz=p, ps=3, cs=1, rgb=p + 256, rps=3, rcs=1, n=8, narrays=38, cfg=ok, out=None, bad=None):
        return L.gsr_scene_from_points(xyz, ps, cs, rgb, rps, rcs, n, narrays,
                                       ctypes.byref(cfg) if cfg is not None else None, out, bad, None)

    for kw in (dict(xyz=None), dict(n=-1), dict(n=INT32_MAX + 1), dict(ps=0), dict(cs=-1), dict(ps=1, cs=1),
               dict(ps=2, cs=1), dict(ps=1, cs=7), dict(rps=0), dict(rcs=0), dict(rps=2, rcs=2), dict(rps=2, rcs=1),
               dict(rps=1, rcs=7), dict(xyz=p + 2), dict(rgb=p + 257), dict(out=p + 514), dict(bad=p + 3),
               dict(narrays=37), dict(narrays=0), dict(narrays=60), dict(cfg=None)):
        assert init(**kw) is None, kw
        err(b"gsr_scene_from_points")
    bad = [dict(opacity=NAN), dict(min_dist2=NAN), dict(scale_mul=NAN), dict(scale_max=NAN), dict(t_center=NAN),
           dict(t_scale=NAN), dict(opacity=0.0), dict(opacity=1.0), dict(opacity=5e-7), dict(opacity=-0.1),
           dict(min_dist2=-1e-9), dict(scale_mul=0.0), dict(scale_mul=-1.0), dict(scale_mul=INF), dict(scale_max=0.0),
           dict(scale_max=-2.0), dict(flags=1), dict(flags=-1)]
    for kw in bad:
        assert init(cfg=good_config(_native, **kw)) is None, kw
        err(b"gsr_scene_from_points")
    for t in (0.0, -1.0):
        assert init(narrays=49, cfg=good_config(_native, t_scale=t)) is None
        err(b"t_scale")
    assert not any(buf)


def test_scratch_bytes(gsr):
    L = gsr.lib()
    assert L.gsr_points_knn_scratch_bytes(0) >= 0
    last = 0
    sweep = sorted(set([1, 2, 3, 63, 64, 65, 4095, 4096, 4097, 262143, 262144, 262145, 10 ** 6, 5 * 10 ** 6, INT32_MAX]
                       + list(range(0, 20000, 61)) + [2 ** k + d for k in range(6, 31) for d in (-1, 0, 1)]))
    for n in sweep:
        b = L.gsr_points_knn_scratch_bytes(n)
        assert b >= last and b >= 0, n
        last = b
    assert 28 * 10 ** 6 <= L.gsr_points_knn_scratch_bytes(10 ** 6) <= 40 * 10 ** 6   # about 32 n
    for n in (-1, -2 ** 40, INT32_MAX + 1, 2 ** 40):
        assert L.gsr_points_knn_scratch_bytes(n) < 0
        assert b"gsr_points_knn_scratch_bytes" in L.gsr_last_error()
        with pytest.raises(gsr.GsrError):
            gsr.points_knn_scratch_bytes(n)
    assert gsr.points_knn_scratch_bytes(1000) == L.gsr_points_knn_scratch_bytes(1000)


def test_python_wrappers_reject_missing_pointers(gsr):
    with pytest.raises(ValueError):
        gsr.points_knn_dist2(None, 8, 0x2000, 0x3000, 4096)
    with pytest.raises(ValueError):
        gsr.points_knn_dist2(0x1000, 8, None, 0x3000, 4096)
    with pytest.raises(ValueError):
        gsr.points_knn_dist2(0x1000, 8, 0x2000, None, 4096)
    with pytest.raises(ValueError):
        gsr.Scene.from_points(None, 8)
    with pytest.raises(ValueError):
        gsr.Scene.from_points(0x1000, 8, narrays=40)
    with pytest.raises(ValueError):
        gsr.Scene(0, 8, owned=False).knn_dist2(0x2000, 0x3000, 4096)
    # an argument error of the library surfaces as GsrError with its message
    with pytest.raises(gsr.GsrError, match="scratch_bytes"):
        gsr.points_knn_dist2(0x1000, 8, 0x2000, 0x3000, 16)
    with pytest.raises(gsr.GsrError, match="overlap"):
        gsr.points_knn_dist2(0x1000, 8, 0x2000, 0x3000, 1 << 20, point_stride=2, comp_stride=1)
    with pytest.raises(gsr.GsrError, match="opacity"):
        gsr.Scene.from_points(0x1000, 8, opacity=1.5)
    with pytest.raises(gsr.GsrError, match="scratch_bytes"):
        gsr.Scene(0x1000, 8, owned=False).knn_dist2(0x2000, 0x3000, 16)
