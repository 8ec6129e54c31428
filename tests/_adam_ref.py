"""The CPU twin of gsr_scene_adam_step (include/gsr.h "scene optimisation") — TEST INFRASTRUCTURE.

A numpy restatement of the step's arithmetic, generic over the dtype.  In float32 every
operation is its own numpy float32 operation (one rounding each, no FMA) and the exp is the
oracle library's orc_expf, the CPU build of gsr_expf: the results are the kernel's bit for bit.
In float64 the exp is np.exp: the same mathematics, which tests/test_adam_ref.py pins to
torch.optim.Adam on the raw (logit / log) parameters.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

PLAIN, EXP, OPACITY = 0, 1, 2
OPACITY_MIN, OPACITY_MAX = np.float32(1e-6), np.float32(0.999999)   # GSR_ADAM_OPACITY_MIN / MAX
GROUP_KEYS = ("position", "opacity", "scale", "rot", "sh", "temporal")   # gsr_scene_grads' pointers
LR_KEYS = ("lr_position", "lr_opacity", "lr_scale", "lr_rot", "lr_sh_dc", "lr_sh_rest", "lr_tcenter", "lr_tscale",
           "lr_motion")


def groups(narrays: int):
    """(pointer key, first plane of the pointer, planes, first block array, lr key, kind) of
    every group a block of `narrays` arrays has."""
    sh_rest = {38: 24, 49: 24, 59: 45}[narrays]
    after_sh = 14 + sh_rest                       # 38, or 59 for an SH-3 block
    g = [("position", 0, 3, 0, "lr_position", PLAIN), ("opacity", 0, 1, 3, "lr_opacity", OPACITY),
         ("scale", 0, 3, 4, "lr_scale", EXP), ("rot", 0, 4, 7, "lr_rot", PLAIN),
         ("sh", 0, 3, 11, "lr_sh_dc", PLAIN), ("sh", 3, sh_rest, 14, "lr_sh_rest", PLAIN)]
    assert after_sh == (59 if narrays == 59 else 38)
    if narrays == 49:
        g += [("temporal", 0, 1, 38, "lr_tcenter", PLAIN), ("temporal", 1, 1, 39, "lr_tscale", EXP),
              ("temporal", 2, 9, 40, "lr_motion", PLAIN)]
    return g


def planes_of(narrays: int):
    """Planes per pointer key."""
    return {"position": 3, "opacity": 1, "scale": 3, "rot": 4, "sh": 48 if narrays == 59 else 27, "temporal": 11}


def orc_exp32(orc):
    """x -> orc_expf(x) elementwise on float32 arrays."""
    f = orc.lib().orc_expf

    def exp32(x):
        x = np.ascontiguousarray(x, np.float32)
        out = np.empty_like(x)
        xf, of = x.ravel(), out.ravel()
        for i in range(xf.size):
            of[i] = f(ctypes.c_float(xf[i]))
        return out
    return exp32


def constants(beta1, beta2, step, dtype):
    """beta1, beta2, omb1, omb2, bc1, bc2 as the host computes them: in double from the betas
    of the working precision, rounded to it."""
    b1, b2 = dtype(beta1), dtype(beta2)
    return (b1, b2, dtype(1.0 - float(b1)), dtype(1.0 - float(b2)),
            dtype(1.0 - math.pow(float(b1), float(step))), dtype(1.0 - math.pow(float(b2), float(step))))


def step_plane(kind, lr, c, eps, g, x, m, v, exp, skip_zero=False):
    """One plane's step: (x', m', v', elements skipped for a non-finite g).  The operation
    order is include/gsr.h's; skipped elements keep x, m and v."""
    dtype = x.dtype.type
    b1, b2, omb1, omb2, bc1, bc2 = c
    one = dtype(1)
    bad = ~np.isfinite(g)
    on = ~bad
    if skip_zero:
        on &= g != 0
    with np.errstate(all="ignore"):
        if kind == OPACITY:
            gp = g * (x * (one - x))
        elif kind == EXP:
            gp = g * x
        else:
            gp = g
        mn = (b1 * m) + (omb1 * gp)
        vn = (b2 * v) + ((omb2 * gp) * gp)
        d = (dtype(lr) * (mn / bc1)) / (np.sqrt(vn / bc2) + dtype(eps))
        if kind == OPACITY:
            xn = x / (x + (one - x) * exp(d))
            xn = np.fmin(np.fmax(xn, dtype(OPACITY_MIN)), dtype(OPACITY_MAX))   # fmaxf / fminf: NaN loses
        elif kind == EXP:
            xn = x * exp(-d)
        else:
            xn = x - d
    for a in (xn, mn, vn):
        assert a.dtype == x.dtype
    return np.where(on, xn, x), np.where(on, mn, m), np.where(on, vn, v), int(bad.sum())


def adam_step(soa, grads, m, v, lrs, step, exp, beta1=0.9, beta2=0.999, eps=1e-15, skip_zero=False,
              zero_grads=False):
    """The whole call on host arrays.  soa: (narrays, n); grads, m, v: dicts of (planes, n)
    arrays by GROUP_KEYS (missing or None: a NULL pointer); lrs: dict by LR_KEYS (missing: 0).
    Returns new (soa, grads, m, v, bad); frozen groups are returned as they came."""
    narrays = soa.shape[0]
    dtype = soa.dtype.type
    c = constants(beta1, beta2, step, dtype)
    soa = soa.copy()
    grads, m, v = ({k: (None if a is None else a.copy()) for k, a in d.items()} for d in (grads, m, v))
    bad = 0
    for key, first, planes, array, lr_key, kind in groups(narrays):
        lr = lrs.get(lr_key, 0.0)
        if grads.get(key) is None or lr == 0:
            continue
        for p in range(planes):
            x, mm, vv, nb = step_plane(kind, lr, c, eps, grads[key][first + p], soa[array + p], m[key][first + p],
                                       v[key][first + p], exp, skip_zero)
            soa[array + p], m[key][first + p], v[key][first + p] = x, mm, vv
            bad += nb
            if zero_grads:
                grads[key][first + p] = 0
    return soa, grads, m, v, bad
