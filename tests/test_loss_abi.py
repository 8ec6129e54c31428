"""The image-loss C ABI (gsr_image_loss, gsr_image_loss_scratch_bytes) on a CPU-only host: the
symbols and their signatures, gsr_loss_config's layout, every argument error (returned before
any device work: the "device" pointers below are host buffers that must never be touched), the
scratch query, and the Python wrappers' checks."""
import ctypes

import pytest

from test_abi import exported_symbols

INT32_MAX = 2 ** 31 - 1


def test_symbols_and_signatures(gsr):
    from gaussianrenderer_amd import _native
    exported = exported_symbols(_native.LIB_PATH)
    sigs = {name: (res, args) for name, res, args in _native.SIGNATURES}
    for name in ("gsr_image_loss", "gsr_image_loss_scratch_bytes"):
        assert name in exported and name in sigs, name
    c_int, c_int64, c_void_p = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    assert sigs["gsr_image_loss_scratch_bytes"] == (c_int64, [c_int, c_int, c_int])
    assert sigs["gsr_image_loss"] == (c_int, [c_void_p, c_void_p, c_int, c_int, ctypes.POINTER(_native.LossConfig),
                                              c_void_p, c_void_p, c_void_p, c_int64, c_void_p])
    # gsr_loss_config: four floats and an int, no padding
    C = _native.LossConfig
    assert [f[0] for f in C._fields_] == ["w_l1", "w_l2", "w_dssim", "grad_scale", "flags"]
    assert [getattr(C, f[0]).offset for f in C._fields_] == [0, 4, 8, 12, 16]
    assert [f[1] for f in C._fields_] == [ctypes.c_float] * 4 + [c_int]
    assert ctypes.sizeof(C) == 20
    assert _native.LOSS_NVALUES == 4
    for name in ("LossConfig", "LOSS_NVALUES", "image_loss", "image_loss_scratch_bytes"):
        assert name in gsr.__all__ and hasattr(gsr, name), name


def test_argument_errors_need_no_device(gsr):
    from gaussianrenderer_amd._native import GSR_E_ARG, LossConfig
    L = gsr.lib()
    W, H = 8, 4
    buf = (ctypes.c_uint64 * 32768)()   # host addresses: the calls below must never touch them
    p = ctypes.addressof(buf)
    image, target, grad, loss, scratch = p, p + 1024, p + 2048, p + 3072, p + 4096
    need_grad = L.gsr_image_loss_scratch_bytes(W, H, 1)
    need_value = L.gsr_image_loss_scratch_bytes(W, H, 0)
    assert 0 < need_value < need_grad <= ctypes.sizeof(buf) - 4096

    def cfg(**over):
        d = dict(w_l1=0.8, w_l2=0.0, w_dssim=0.2, grad_scale=1.0, flags=0)
        d.update(over)
        return LossConfig(**d)

    def call(x=image, y=target, w=W, h=H, c=None, g=grad, l=loss, s=scratch, nbytes=need_grad, null_cfg=False):
        c = c or cfg()
        return L.gsr_image_loss(x, y, w, h, None if null_cfg else ctypes.byref(c), g, l, s, nbytes, None)

    inf, nan = float("inf"), float("nan")
    cases = {
        "null image": dict(x=None),
        "null target": dict(y=None),
        "null cfg": dict(null_cfg=True),
        "both outputs null": dict(g=None, l=None),
        "W = 0": dict(w=0),
        "W < 0": dict(w=-8),
        "H = 0": dict(h=0),
        "H < 0": dict(h=-1),
        "3 W H > INT32_MAX": dict(w=32768, h=21846, nbytes=2 ** 62),
        "W H overflows int32": dict(w=65536, h=65536, nbytes=2 ** 62),
        "negative w_l1": dict(c=cfg(w_l1=-0.8)),
        "negative w_l2": dict(c=cfg(w_l2=-1e-3)),
        "negative w_dssim": dict(c=cfg(w_dssim=-0.2)),
        "infinite w_l1": dict(c=cfg(w_l1=inf)),
        "NaN w_l2": dict(c=cfg(w_l2=nan)),
        "NaN w_dssim": dict(c=cfg(w_dssim=nan)),
        "every weight 0": dict(c=cfg(w_l1=0.0, w_l2=0.0, w_dssim=0.0)),
        "infinite grad_scale": dict(c=cfg(grad_scale=inf)),
        "NaN grad_scale": dict(c=cfg(grad_scale=nan)),
        "unknown flag": dict(c=cfg(flags=1)),
        "unknown high flag": dict(c=cfg(flags=1 << 30)),
        "null scratch": dict(s=None),
        "scratch one byte short": dict(nbytes=need_grad - 1),
        "the value-only size with a gradient": dict(nbytes=need_value),
        "value-only scratch one byte short": dict(g=None, nbytes=need_value - 1),
        "scratch_bytes = 0": dict(nbytes=0),
        "scratch_bytes < 0": dict(nbytes=-1),
        "misaligned image": dict(x=image + 2),
        "misaligned target": dict(y=target + 1),
        "misaligned gradient": dict(g=grad + 3),
        "misaligned loss": dict(l=loss + 2),
        "misaligned scratch": dict(s=scratch + 1),
        "gradient is the image": dict(g=image),
        "gradient is the target": dict(g=target),
    }
    assert 3 * 32768 * 21846 > INT32_MAX >= 3 * 32768 * 21845
    for name, kw in cases.items():
        assert call(**kw) == GSR_E_ARG, name
        msg = L.gsr_last_error()
        assert msg and b"gsr_image_loss" in msg, name
    assert not any(buf)


def test_scratch_query(gsr):
    from gaussianrenderer_amd._native import GSR_E_ARG
    L = gsr.lib()
    q = L.gsr_image_loss_scratch_bytes
    sizes = [(1, 1), (300, 1), (17, 17), (16, 32), (70, 5), (130, 33), (1600, 1063), (1920, 1080), (32768, 21845)]
    sizes.sort(key=lambda wh: wh[0] * wh[1])
    last = (0, 0)
    for W, H in sizes:
        value, grad = q(W, H, 0), q(W, H, 1)
        assert 0 < value <= grad, (W, H)
        assert q(W, H, 7) == grad                      # want_grad is a truth value
        assert q(H, W, 1) == grad and q(H, W, 0) == value
        assert value >= last[0] and grad >= last[1], f"not monotone in W*H at {W}x{H}"
        last = (value, grad)
    for W, H in ((0, 4), (4, 0), (-1, 4), (4, -1), (32768, 21846), (65536, 65536), (INT32_MAX, INT32_MAX)):
        for want in (0, 1):
            assert q(W, H, want) == GSR_E_ARG, (W, H)
            assert b"gsr_image_loss_scratch_bytes" in L.gsr_last_error()
    assert gsr.image_loss_scratch_bytes(1920, 1080) == q(1920, 1080, 1)
    assert gsr.image_loss_scratch_bytes(1920, 1080, want_grad=False) == q(1920, 1080, 0)
    with pytest.raises(gsr.GsrError):
        gsr.image_loss_scratch_bytes(0, 1080)


def test_python_wrapper_checks(gsr):
    # never dereferenced: the wrapper or the native argument check raises first
    x, y, g, l, s = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
    with pytest.raises(ValueError):
        gsr.image_loss(None, y, 8, 4, grad_ptr=g, scratch_ptr=s)
    with pytest.raises(ValueError):
        gsr.image_loss(x, None, 8, 4, grad_ptr=g, scratch_ptr=s)
    with pytest.raises(ValueError):                       # neither output
        gsr.image_loss(x, y, 8, 4, scratch_ptr=s)
    with pytest.raises(ValueError):
        gsr.image_loss(x, y, 8, 4, grad_ptr=g, loss_ptr=l, scratch_ptr=None)
    with pytest.raises(TypeError):                        # scratch_ptr has no default
        gsr.image_loss(x, y, 8, 4, grad_ptr=g)
    with pytest.raises(TypeError):                        # the weights are keyword-only
        gsr.image_loss(x, y, 8, 4, 0.8, 0.0, 0.2, grad_ptr=g, scratch_ptr=s)

    class T:   # anything with .data_ptr() is accepted as a pointer; 0 is a missing one
        def data_ptr(self):
            return 0
    with pytest.raises(ValueError):
        gsr.image_loss(T(), y, 8, 4, grad_ptr=g, scratch_ptr=s)
    with pytest.raises(ValueError):
        gsr.image_loss(x, y, 8, 4, grad_ptr=T(), scratch_ptr=s)
    # what the native call refuses arrives as GsrError, not as a crash
    with pytest.raises(gsr.GsrError):
        gsr.image_loss(x, y, 8, 4, w_l1=-1.0, grad_ptr=g, scratch_ptr=s)
    with pytest.raises(gsr.GsrError):
        gsr.image_loss(x, y, 8, 4, w_l1=0.0, w_dssim=0.0, loss_ptr=l, scratch_ptr=s)
    with pytest.raises(gsr.GsrError):
        gsr.image_loss(x, y, 8, 4, grad_ptr=x, scratch_ptr=s)
    with pytest.raises(gsr.GsrError):                     # the value-only size does not do for a gradient
        gsr.image_loss(x, y, 8, 4, grad_ptr=g, scratch_ptr=s, scratch_bytes=gsr.image_loss_scratch_bytes(8, 4, False))
    with pytest.raises(gsr.GsrError):
        gsr.image_loss(x, y, 0, 4, grad_ptr=g, scratch_ptr=s, scratch_bytes=1 << 20)
