"""The scene-editing C ABI (gsr_mask_indices, gsr_gather_planes, gsr_scene_gather,
gsr_scene_select) on a CPU-only host: the symbols, the argument errors (returned before any
device work: the "device" pointers below are host buffers that must never be touched) and
the Python wrappers' argument checks."""
import ctypes

import pytest

from test_abi import exported_symbols

NAMES = ("gsr_mask_indices", "gsr_gather_planes", "gsr_scene_gather", "gsr_scene_select")
INT32_MAX = 2 ** 31 - 1


def test_symbols_and_signatures(gsr):
    from gaussianrenderer_amd import _native
    syms = exported_symbols(_native.LIB_PATH)
    sigs = {name for name, _, _ in _native.SIGNATURES}
    for name in NAMES:
        assert name in syms and name in sigs, name
    assert hasattr(gsr.Scene, "select") and hasattr(gsr.Scene, "gather")
    assert "mask_indices" in gsr.__all__ and "gather_planes" in gsr.__all__


def test_argument_errors_need_no_device(gsr):
    from gaussianrenderer_amd._native import GSR_E_ARG
    L = gsr.lib()
    buf = (ctypes.c_uint64 * 64)()   # a host address: the calls below must never touch it
    p = ctypes.addressof(buf)
    m = ctypes.c_int64(-7)

    def err():
        msg = L.gsr_last_error()
        assert msg, "no message"
        return msg

    # gsr_mask_indices(d_keep, n, d_indices, m_out, stream)
    for args in ((None, 8, p, ctypes.byref(m), None), (p, 8, None, ctypes.byref(m), None), (p, 8, p, None, None),
                 (p, -1, p, ctypes.byref(m), None), (p, INT32_MAX + 1, p, ctypes.byref(m), None)):
        assert L.gsr_mask_indices(*args) == GSR_E_ARG, args
        assert b"gsr_mask_indices" in err()
    assert m.value == -7

    # gsr_gather_planes(d_dst, dst_stride, d_src, src_stride, nplanes, elem_bytes, n, d_indices, m, d_bad, stream)
    def gp(dst=p, ds=8, src=p + 256, ss=8, nplanes=2, eb=4, n=8, idx=p + 128, mm=8, bad=None):
        return L.gsr_gather_planes(dst, ds, src, ss, nplanes, eb, n, idx, mm, bad, None)

    for kw in (dict(dst=None), dict(src=None), dict(idx=None), dict(eb=0), dict(eb=2), dict(eb=16), dict(eb=-4),
               dict(nplanes=0), dict(nplanes=-3), dict(n=-1), dict(mm=-1), dict(ss=7), dict(ds=7),
               dict(mm=INT32_MAX + 1, ds=INT32_MAX + 1), dict(n=INT32_MAX + 1, ss=INT32_MAX + 1),
               dict(n=0, ss=0, mm=1)):
        assert gp(**kw) == GSR_E_ARG, kw
        assert b"gsr_gather_planes" in err()

    # gsr_scene_gather(d_scene, narrays, n, d_indices, m, d_bad, stream)
    for args in ((None, 38, 8, p, 4, None, None), (p, 38, 8, None, 4, None, None), (p, 37, 8, p, 4, None, None),
                 (p, 0, 8, p, 4, None, None), (p, 38, -1, p, 4, None, None), (p, 38, 8, p, -1, None, None),
                 (p, 38, 8, p, INT32_MAX + 1, None, None), (p, 49, 0, p, 1, None, None)):
        assert L.gsr_scene_gather(*args) is None, args
        err()

    # gsr_scene_select(d_scene, narrays, n, d_keep, m_out, d_indices, stream)
    for args in ((None, 38, 8, p, ctypes.byref(m), None, None), (p, 38, 8, None, ctypes.byref(m), None, None),
                 (p, 38, 8, p, None, None, None), (p, 50, 8, p, ctypes.byref(m), None, None),
                 (p, 59, -2, p, ctypes.byref(m), p, None), (p, 59, INT32_MAX + 1, p, ctypes.byref(m), p, None)):
        assert L.gsr_scene_select(*args) is None, args
        err()
    assert m.value == -7
    assert not any(buf)


def test_mask_indices_of_nothing(gsr):
    m = ctypes.c_int64(-7)
    assert gsr.lib().gsr_mask_indices(None, 0, None, ctypes.byref(m), None) == 0
    assert m.value == 0
    assert gsr.mask_indices(None, 0, None) == 0


def test_python_wrappers_reject_missing_pointers(gsr):
    s = gsr.Scene(0x1000, 8, owned=False)   # never dereferenced: the wrappers raise first
    with pytest.raises(ValueError):
        s.select(None)
    with pytest.raises(ValueError):
        s.select(0)
    with pytest.raises(ValueError):
        s.gather(None, 4)
    with pytest.raises(ValueError):
        s.gather(0, 4)
    with pytest.raises(ValueError):
        gsr.mask_indices(None, 8, 0x2000)
    with pytest.raises(ValueError):
        gsr.mask_indices(0x2000, 8, None)
    with pytest.raises(ValueError):
        gsr.gather_planes(0x1000, 8, 0x2000, 8, 1, 4, 8, None, 8)
    with pytest.raises(ValueError):
        gsr.gather_planes(None, 8, 0x2000, 8, 1, 4, 8, 0x3000, 8)

    class T:   # anything with .data_ptr() is accepted as a pointer
        def data_ptr(self):
            return 0
    with pytest.raises(ValueError):
        gsr.mask_indices(T(), 8, T())
