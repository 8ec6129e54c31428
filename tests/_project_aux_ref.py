"""Reference of gsr_project_backward_aux (include/gsr.h) — TEST INFRASTRUCTURE.

tests/_project_ref.py's float64 torch restatement with an eleventh record component, -Z = minus
the view position's z, behind the ten of gsr_project_backward.  Gradients are torch.autograd's;
scales, validity and the ambiguous Gaussians are _project_ref's (the depth adds no decision of
its own).
"""
from __future__ import annotations

import numpy as np
import torch

import _project_ref as pr

REC_ROWS = dict(pr.REC_ROWS, z=slice(10, 11))
INPUTS = ("color", "opacity", "conic", "center", "z")


def record(f):
    """The eleven record components (11, m) of a _project_ref.forward()."""
    return torch.cat([f["color"], f["opacity"][None], f["conic"], f["center"], -f["view"][2:3]])


def evaluate(soa, camv, W, H, t=0.0, upstream=None, dtype=torch.float64, valid=None):
    """_project_ref.evaluate with upstream (11, n): "grad" (narrays, n) = sum_c VJP_c and "abs"
    = sum_c |VJP_c| over the eleven components, zero at Gaussians that are not valid."""
    soa = np.ascontiguousarray(soa)
    narrays, n = soa.shape
    first = pr.evaluate(soa, camv, W, H, t, valid=valid)
    valid = first["valid"]
    idx = np.flatnonzero(valid)
    x = torch.from_numpy(soa[:, idx].astype(np.float64)).to(dtype).requires_grad_(True)
    rec = record(pr.forward(x, camv, W, H, t))
    up = torch.from_numpy(np.asarray(upstream, np.float64)[:, idx]).to(dtype)
    grad, absg = np.zeros((narrays, n), np.float64), np.zeros((narrays, n), np.float64)
    for c in range(11):
        if not up[c].any():
            continue
        (g,) = torch.autograd.grad((rec[c] * up[c]).sum(), x, retain_graph=True)
        g = g.numpy().astype(np.float64)
        grad[:, idx] += g
        absg[:, idx] += np.abs(g)
    return {"valid": valid, "ambiguous": first["ambiguous"], "grad": grad, "abs": absg}


def central_difference(soa, camv, W, H, t, upstream, j, i, rel=1e-6):
    """d/d soa[j, i] of sum_c upstream[c, i] record[c, i], by a central difference of the float64
    forward of Gaussian i alone."""
    col = np.asarray(soa[:, i:i + 1], np.float64)
    h = rel * max(abs(col[j, 0]), 1e-2)
    vals = []
    for s in (+1.0, -1.0):
        cpy = col.copy()
        cpy[j, 0] += s * h
        with torch.no_grad():
            rec = record(pr.forward(torch.from_numpy(cpy), camv, W, H, t)).numpy()[:, 0]
        vals.append(rec * np.asarray(upstream, np.float64)[:, i])
    return float((vals[0] - vals[1]).sum()) / (2 * h)     # differenced per component, then summed


# (case of _project_ref.CASES, mode): a 38-array block with random quaternions, an SH-3 block, a
# 4D block, and a camera inside the cloud (hundreds of culled Gaussians); "z": d_z alone,
# "mixed": all eleven planes
RUNS = [(case, mode) for case in ("rot", "sh3", "4d", "sparse_in") for mode in ("z", "mixed")]

_refs = {}


def reference(gsr, tmp_path_factory, case, mode):
    """The float64 reference of one run, computed once and left unchanged: evaluate()'s dict plus
    "soa", "camv", "upstream" (11, n) float32 — standard normal on ALL n Gaussians, rows 0..9
    zero in mode "z", then zeroed at the ambiguous Gaussians (and, on a 4D block, the opacity's
    where the temporal factor underflows: _project_ref.reference) — and "A" (narrays, n)."""
    key = (case, mode)
    if key not in _refs:
        c = pr.CASES[case]
        base = pr.reference(gsr, tmp_path_factory, case)
        soa, camv = base["soa"], base["camv"]
        n = soa.shape[1]
        up = np.random.default_rng(500 + pr.SEEDS[case]).standard_normal((11, n)).astype(np.float32)
        if mode == "z":
            up[:10] = 0.0
        up[:, base["ambiguous"]] = 0.0
        up[3, base["underflow"]] = 0.0
        res = evaluate(soa, camv, c["W"], c["H"], c.get("time", 0.0), upstream=up, valid=base["valid"])
        res["ambiguous"] = base["ambiguous"]
        res.update(soa=soa, camv=camv, upstream=up, A=pr.scale(res["abs"], soa.shape[0]))
        for v in res.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _refs[key] = res
    return _refs[key]
