"""The scene-optimisation C ABI (gsr_scene_adam_step) on a CPU-only host: the symbol and its
signature, every argument error (returned before any device work: the "device" pointers below
are host buffers that must never be touched), n == 0, and the Python wrapper's checks."""
import ctypes

import pytest

from test_abi import exported_symbols

INT32_MAX = 2 ** 31 - 1
LAYOUT_BLOCK, LAYOUT_AOS, LAYOUT_4D, LAYOUT_SH3 = 0, 1, 2, 3


def test_symbol_and_signature(gsr):
    from gaussianrenderer_amd import _native
    assert "gsr_scene_adam_step" in exported_symbols(_native.LIB_PATH)
    sig = {name: (res, args) for name, res, args in _native.SIGNATURES}["gsr_scene_adam_step"]
    assert sig[0] is ctypes.c_int and len(sig[1]) == 9
    assert sig[1][3] == sig[1][4] == sig[1][5] == ctypes.POINTER(_native.SceneGrads)
    assert sig[1][6] == ctypes.POINTER(_native.AdamConfig)
    # gsr_adam_config: nine lrs, two betas and eps (12 floats), an aligned int64 step, an int
    C = _native.AdamConfig
    assert [f[0] for f in C._fields_] == ["lr_position", "lr_opacity", "lr_scale", "lr_rot", "lr_sh_dc", "lr_sh_rest",
                                         "lr_tcenter", "lr_tscale", "lr_motion", "beta1", "beta2", "eps", "step",
                                         "flags"]
    assert (C.eps.offset, C.step.offset, C.flags.offset, ctypes.sizeof(C)) == (44, 48, 56, 64)
    assert (_native.ADAM_SKIP_ZERO, _native.ADAM_ZERO_GRADS) == (1, 2)
    assert hasattr(gsr.Scene, "adam_step")
    for name in ("AdamConfig", "ADAM_SKIP_ZERO", "ADAM_ZERO_GRADS", "SCENE_GRAD_GROUPS"):
        assert name in gsr.__all__ and hasattr(gsr, name), name


def test_argument_errors_need_no_device(gsr):
    from gaussianrenderer_amd._native import GSR_E_ARG, AdamConfig, SceneGrads
    L = gsr.lib()
    buf = (ctypes.c_uint64 * 4096)()   # host addresses: the calls below must never touch them
    p = ctypes.addressof(buf)
    n = 8

    def sg(base, **over):
        """Six planes' worth of distinct addresses inside buf; over: a field -> another value."""
        d = dict(d_position=base, d_opacity=base + 256, d_scale=base + 512, d_rot=base + 768, d_sh=base + 1024,
                 d_temporal=None)
        d.update(over)
        return SceneGrads(**d)

    def cfg(**over):
        d = dict(lr_position=1e-3, lr_opacity=1e-2, lr_scale=1e-3, lr_rot=1e-3, lr_sh_dc=1e-3, lr_sh_rest=1e-4,
                 lr_tcenter=0.0, lr_tscale=0.0, lr_motion=0.0, beta1=0.9, beta2=0.999, eps=1e-15, step=1, flags=0)
        d.update(over)
        return AdamConfig(**d)

    def call(scene=p, layout=LAYOUT_BLOCK, nn=n, g=None, m=None, v=None, c=None, bad=None, null=()):
        g = g or sg(p + 2048)
        m = m or sg(p + 8192)
        v = v or sg(p + 16384)
        c = c or cfg()
        args = dict(g=ctypes.byref(g), m=ctypes.byref(m), v=ctypes.byref(v), c=ctypes.byref(c))
        for k in null:
            args[k] = None
        return L.gsr_scene_adam_step(scene, layout, nn, args["g"], args["m"], args["v"], args["c"], bad, None)

    inf, nan = float("inf"), float("nan")
    t_lrs = dict(lr_tcenter=1e-3, lr_tscale=1e-3, lr_motion=1e-3)
    cases = {
        "null scene, n > 0": dict(scene=None),
        "null grads": dict(null=("g",)),
        "null m": dict(null=("m",)),
        "null v": dict(null=("v",)),
        "null cfg": dict(null=("c",)),
        "AoS": dict(layout=LAYOUT_AOS),
        "unknown layout": dict(layout=4),
        "negative layout": dict(layout=-1),
        "n < 0": dict(nn=-1),
        "n > INT32_MAX": dict(nn=INT32_MAX + 1),
        "no gradient pointer": dict(g=SceneGrads()),
        "every lr 0": dict(c=cfg(lr_position=0, lr_opacity=0, lr_scale=0, lr_rot=0, lr_sh_dc=0, lr_sh_rest=0)),
        "the only pointer's lr 0": dict(g=SceneGrads(d_rot=p + 2048), c=cfg(lr_rot=0)),
        "active group without m": dict(m=sg(p + 8192, d_scale=None)),
        "active group without v": dict(v=sg(p + 16384, d_opacity=None)),
        "sh_rest alone active without v": dict(v=sg(p + 16384, d_sh=None), c=cfg(lr_sh_dc=0)),
        "temporal on a 3D block": dict(g=sg(p + 2048, d_temporal=p + 4096), m=sg(p + 8192, d_temporal=p + 12288),
                                       v=sg(p + 16384, d_temporal=p + 20480), c=cfg(**t_lrs)),
        "temporal on an SH-3 block": dict(layout=LAYOUT_SH3, g=sg(p + 2048, d_temporal=p + 4096),
                                          m=sg(p + 8192, d_temporal=p + 12288), v=sg(p + 16384, d_temporal=p + 20480),
                                          c=cfg(lr_motion=1e-3)),
        "temporal without moments on a 4D block": dict(layout=LAYOUT_4D, g=sg(p + 2048, d_temporal=p + 4096),
                                                       c=cfg(lr_tscale=1e-3)),
        "negative lr": dict(c=cfg(lr_scale=-1e-3)),
        "negative lr of a frozen group": dict(c=cfg(lr_motion=-1.0)),
        "infinite lr": dict(c=cfg(lr_position=inf)),
        "NaN lr": dict(c=cfg(lr_sh_rest=nan)),
        "beta1 = 1": dict(c=cfg(beta1=1.0)),
        "beta1 < 0": dict(c=cfg(beta1=-0.1)),
        "beta1 NaN": dict(c=cfg(beta1=nan)),
        "beta2 = 1": dict(c=cfg(beta2=1.0)),
        "beta2 < 0": dict(c=cfg(beta2=-1e-3)),
        "eps = 0": dict(c=cfg(eps=0.0)),
        "eps < 0": dict(c=cfg(eps=-1e-8)),
        "eps infinite": dict(c=cfg(eps=inf)),
        "eps NaN": dict(c=cfg(eps=nan)),
        "step = 0": dict(c=cfg(step=0)),
        "step < 0": dict(c=cfg(step=-5)),
        "unknown flag": dict(c=cfg(flags=4)),
        "unknown flag beside known ones": dict(c=cfg(flags=3 | 8)),
        "misaligned scene": dict(scene=p + 2),
        "misaligned gradient": dict(g=sg(p + 2048, d_rot=p + 2048 + 769)),
        "misaligned m": dict(m=sg(p + 8192, d_position=p + 8193)),
        "misaligned v": dict(v=sg(p + 16384, d_sh=p + 16386)),
        "misaligned d_bad": dict(bad=p + 30001),
    }
    for name, kw in cases.items():
        assert call(**kw) == GSR_E_ARG, name
        msg = L.gsr_last_error()
        assert msg and b"gsr_scene_adam_step" in msg, name
    # a frozen group needs no moments, and a frozen d_temporal may be given for a 3D block:
    # with n == 0 such calls are accepted, without device work
    assert call(nn=0, m=sg(p + 8192, d_rot=None), v=sg(p + 16384, d_rot=None), c=cfg(lr_rot=0)) == 0
    assert call(nn=0, g=sg(p + 2048, d_temporal=p + 4096)) == 0
    assert not any(buf)


def test_step_of_nothing(gsr):
    """n == 0 is GSR_OK without device work, with or without a scene pointer; the other
    arguments are still checked."""
    from gaussianrenderer_amd._native import GSR_E_ARG, AdamConfig, SceneGrads
    L = gsr.lib()
    buf = (ctypes.c_uint64 * 64)()
    p = ctypes.addressof(buf)
    g, m, v = SceneGrads(d_position=p), SceneGrads(d_position=p + 64), SceneGrads(d_position=p + 128)
    c = AdamConfig(lr_position=1e-3, beta1=0.9, beta2=0.999, eps=1e-15, step=1, flags=3)
    for scene in (None, p + 256):
        for layout in (LAYOUT_BLOCK, LAYOUT_4D, LAYOUT_SH3):
            assert L.gsr_scene_adam_step(scene, layout, 0, ctypes.byref(g), ctypes.byref(m), ctypes.byref(v),
                                         ctypes.byref(c), None, None) == 0
    c.step = 0
    assert L.gsr_scene_adam_step(None, LAYOUT_BLOCK, 0, ctypes.byref(g), ctypes.byref(m), ctypes.byref(v),
                                 ctypes.byref(c), None, None) == GSR_E_ARG
    assert not any(buf)
    # and through the wrapper
    gsr.Scene(0, 0, owned=False).adam_step({"position": p}, {"position": p + 64}, {"position": p + 128},
                                           step=1, lr_position=1e-3)
    assert not any(buf)


def test_python_wrapper_rejects_missing_pointers(gsr):
    s = gsr.Scene(0x1000, 8, owned=False)   # never dereferenced: the wrapper raises first
    g, m, v = {"position": 0x2000, "sh": 0x3000}, {"position": 0x4000, "sh": 0x5000}, {"position": 0x6000, "sh": 0x7000}
    with pytest.raises(ValueError):
        s.adam_step(None, m, v, step=1, lr_position=1e-3)
    with pytest.raises(ValueError):
        s.adam_step(g, None, v, step=1, lr_position=1e-3)
    with pytest.raises(ValueError):
        s.adam_step(g, m, None, step=1, lr_position=1e-3)
    with pytest.raises(ValueError):                       # no group: every lr 0
        s.adam_step(g, m, v, step=1)
    with pytest.raises(ValueError):                       # no group: the lr's gradient is missing
        s.adam_step(g, m, v, step=1, lr_opacity=1e-2)
    with pytest.raises(ValueError):                       # an active group without m
        s.adam_step(g, {"sh": 0x5000}, v, step=1, lr_position=1e-3)
    with pytest.raises(ValueError):                       # sh_rest alone active, without v
        s.adam_step(g, m, {"position": 0x6000}, step=1, lr_sh_rest=1e-3)
    with pytest.raises(ValueError):                       # an unknown group name
        s.adam_step({"colour": 0x2000}, m, v, step=1, lr_position=1e-3)
    with pytest.raises(ValueError):                       # a sequence must name all six
        s.adam_step([0x2000, 0x3000], m, v, step=1, lr_position=1e-3)
    with pytest.raises(TypeError):                        # step has no default
        s.adam_step(g, m, v, lr_position=1e-3)

    class T:   # anything with .data_ptr() is accepted as a pointer; 0 is a missing one
        def data_ptr(self):
            return 0
    with pytest.raises(ValueError):
        s.adam_step({"position": T()}, m, v, step=1, lr_position=1e-3)
    with pytest.raises(ValueError):
        s.adam_step(g, {"position": T()}, v, step=1, lr_position=1e-3)
    # what the native call refuses arrives as GsrError, not as a crash
    with pytest.raises(gsr.GsrError):
        s.adam_step(g, m, v, step=0, lr_position=1e-3)
    with pytest.raises(gsr.GsrError):
        s.adam_step(g, m, v, step=1, lr_position=-1e-3)
