"""Reference of gsr_project_backward (include/gsr.h) — TEST INFRASTRUCTURE.

A torch restatement of the preprocess's map from scene arrays to splat record (position ->
view -> clip -> ndc -> centre; quaternion and scales -> covariance -> 2D conic; SH -> colour;
temporal opacity), on CPU tensors, in float64 (the yardstick) or float32 (to measure what
single precision alone costs).  The gradients are torch.autograd's: nothing here is derived by
hand, which is what the hand-derived kernel is checked against.

One backward run per record component (ten), each with that component's upstream plane alone,
gives VJP_c (narrays, n).  The reference gradient is their sum; the SCALE of output group G
(position, opacity, scale, rot, sh, temporal) and Gaussian i is
    A[G, i] = max over the arrays j of G of sum_c |VJP_c[j, i]|
and errors are |got - ref| / A.  Per group, not per array: an SH basis term such as 2zz - xx -
yy, or a quaternion component, cancels internally, and its own magnitude hides that.

Decisions float32 could take either way are not compared: the upstream is zeroed on both sides
at a Gaussian whose unclamped colour lies within 1e-5 of a clamp bound, or whose Z, ndc z or
det lies within a relative 1e-4 of its threshold.
"""
from __future__ import annotations

import numpy as np
import torch

RING_COLOR, RING_REL = 1e-5, 1e-4
AMBIGUOUS_SHARE_CAP = 0.02
DET_MIN = 1e-8
TFAC_MIN = 1e-30

C0, C1 = 0.28209479177387814, 0.4886025119029199
C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
      1.445305721320277, -0.5900435899266435)

RECORD = (("color", 3), ("opacity", 1), ("conic", 4), ("center", 2))       # the ten upstream planes, in order
REC_ROWS = {"color": slice(0, 3), "opacity": slice(3, 4), "conic": slice(4, 8), "center": slice(8, 10)}


def groups(narrays):
    """name -> rows of the scene block (= planes of the gradient block) of each output group."""
    g = {"position": slice(0, 3), "opacity": slice(3, 4), "scale": slice(4, 7), "rot": slice(7, 11),
         "sh": slice(11, 59 if narrays == 59 else 38)}
    if narrays == 49:
        g["temporal"] = slice(38, 49)
    return g


def camera_values(gsr, cam):
    """What the preprocess reads of a camera, as exact float64 copies of its float32 values."""
    from gaussianrenderer_amd import camera_intrinsics
    fx, fy = camera_intrinsics(cam)
    f = lambda a, shape: np.array(list(a), np.float32).astype(np.float64).reshape(shape)  # noqa: E731
    return {"V": f(cam.V_matrix, (4, 4)), "P": f(cam.P_matrix, (4, 4)), "Rc": f(cam.r_cam, (3, 3)),
            "RcT": f(cam.r_cam_T, (3, 3)), "campos": f(cam.position, (3,)), "znear": float(np.float32(cam.nearClip)),
            "fx": float(np.float32(fx)), "fy": float(np.float32(fy))}


def sh_basis(d, ncoef):
    """[B_0 .. B_ncoef-1] at the unit directions d (3, m): render.cu:500-534, band 3 as 3DGS."""
    x, y, z = d[0], d[1], d[2]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    B = [torch.full_like(x, C0), -C1 * y, C1 * z, -C1 * x,
         C2[0] * xy, C2[1] * yz, C2[2] * (2.0 * zz - xx - yy), C2[3] * xz, C2[4] * (xx - yy)]
    if ncoef == 16:
        B += [C3[0] * y * (3.0 * xx - yy), C3[1] * xy * z, C3[2] * y * (4.0 * zz - xx - yy),
              C3[3] * z * (2.0 * zz - 3.0 * xx - 3.0 * yy), C3[4] * x * (4.0 * zz - xx - yy), C3[5] * z * (xx - yy),
              C3[6] * x * (xx - 3.0 * yy)]
    return B


def forward(soa, camv, W, H, t=0.0):
    """The record of every Gaussian of soa (narrays, m), a torch tensor of the dtype to compute
    in.  Returns color (3, m; clamped), raw (3, m; unclamped), opacity (m), conic (4, m), center
    (2, m; NOT rounded), view (4, m), ndc (3, m), det (m).  Invalid Gaussians give whatever the
    formulas give (inf, nan): callers select the valid ones first."""
    dt_ = soa.dtype
    c = {k: torch.as_tensor(v, dtype=dt_) for k, v in camv.items()}
    narrays = soa.shape[0]
    p = soa[0:3]
    opacity = soa[3]
    if narrays == 49:
        dt = t - soa[38]
        m = soa[40:49]
        p = p + m[0:3] * dt + m[3:6] * (dt * dt) + m[6:9] * (dt * dt * dt)
        opacity = opacity * torch.exp(-(dt / soa[39]) ** 2)
    one = torch.ones_like(p[:1])
    view = c["V"] @ torch.cat([p, one])                     # (4, m)
    clip = c["P"] @ view
    ndc = clip[0:3] / clip[3:4]
    center = torch.stack([(ndc[0] + 1.0) * (W * 0.5), (ndc[1] + 1.0) * (H * 0.5)])
    # covariance
    q = soa[7:11]
    u = q / torch.sqrt((q * q).sum(0, keepdim=True))
    w, x, y, z = u[0], u[1], u[2], u[3]
    R = torch.stack([torch.stack([1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * w * z, 2 * x * z + 2 * w * y]),
                     torch.stack([2 * x * y + 2 * w * z, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * w * x]),
                     torch.stack([2 * x * z - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x * x - 2 * y * y])])   # (3, 3, m)
    N = R * soa[4:7][None]                                   # N[i, j] = R[i, j] s[j]
    Sigma = torch.einsum("ikm,jkm->ijm", N, N)
    Sc = torch.einsum("ik,klm,lj->ijm", c["Rc"], Sigma, c["RcT"])
    X, Y, Z = view[0], view[1], view[2]
    zero = torch.zeros_like(X)
    J = torch.stack([torch.stack([c["fx"] / Z, zero, -c["fx"] * X / (Z * Z)]),
                     torch.stack([zero, c["fy"] / Z, -c["fy"] * Y / (Z * Z)])])                             # (2, 3, m)
    T = torch.einsum("ikm,klm,jlm->ijm", J, Sc, J)
    D = torch.tensor([[(W * 0.5) ** 2, (W * 0.5) * (H * 0.5)], [(H * 0.5) * (W * 0.5), (H * 0.5) ** 2]], dtype=dt_)
    M = D[:, :, None] * T
    det = M[0, 0] * M[1, 1] - M[0, 1] * M[1, 0]
    conic = torch.stack([M[1, 1], -M[0, 1], -M[1, 0], M[0, 0]]) / det
    # colour
    d = p - c["campos"][:, None]
    nn = torch.sqrt((d * d).sum(0))
    far = nn > 1e-8
    d = torch.where(far, d / torch.where(far, nn, torch.ones_like(nn)), torch.zeros_like(d))
    ncoef = 16 if narrays == 59 else 9
    B = sh_basis(d, ncoef)
    sh = soa[11:11 + 3 * ncoef].reshape(ncoef, 3, -1)
    raw = sum(B[k][None] * sh[k] for k in range(ncoef)) + 0.5
    inside = (raw > 0) if ncoef == 16 else ((raw > 0) & (raw < 1))
    hi = torch.full_like(raw, float("inf")) if ncoef == 16 else torch.ones_like(raw)
    color = torch.where(inside, raw, torch.minimum(torch.clamp(raw.detach(), min=0.0), hi))
    return {"color": color, "raw": raw, "opacity": opacity, "conic": conic, "center": center, "view": view,
            "ndc": ndc, "det": det}


def validity(f, znear, sh3):
    """(valid, ambiguous) of a float64 forward(): the preprocess's tests (render.cu:543-556,
    690), and the Gaussians a float32 evaluation might decide differently or clamp differently."""
    view, ndc, det, raw = (f[k].detach().numpy() for k in ("view", "ndc", "det", "raw"))
    with np.errstate(invalid="ignore"):
        finite = np.isfinite(view[:3]).all(0) & np.isfinite(ndc).all(0) & np.isfinite(det)
        valid = finite & ~(view[2] >= -znear) & ~(ndc[2] < -1.0) & ~(ndc[2] > 1.0) & ~(det < DET_MIN)
        amb = (np.abs(view[2] + znear) <= RING_REL * znear) | (np.abs(np.abs(ndc[2]) - 1.0) <= RING_REL) | \
              (np.abs(det - DET_MIN) <= RING_REL * DET_MIN)
        ring = np.abs(raw) <= RING_COLOR
        if not sh3:      # an SH-3 block clamps at 0 only
            ring |= np.abs(raw - 1.0) <= RING_COLOR
        amb_color = valid & ring.any(0)
    return valid, (amb & finite) | amb_color


def evaluate(soa, camv, W, H, t=0.0, upstream=None, dtype=torch.float64, valid=None):
    """Forward and, with upstream (10, n), the gradients.  valid: the set to evaluate (default:
    this evaluation's own float64 validity).  Returns the forward fields as numpy (n columns, nan
    where not valid), "valid", "ambiguous" and, with upstream, "grad" (narrays, n) = sum_c VJP_c
    and "abs" (narrays, n) = sum_c |VJP_c|, zero at Gaussians that are not valid."""
    soa = np.ascontiguousarray(soa)
    narrays, n = soa.shape
    if valid is None:
        with torch.no_grad():
            f = forward(torch.from_numpy(soa.astype(np.float64)), camv, W, H, t)
        valid, amb = validity(f, camv["znear"], narrays == 59)
    else:
        amb = np.zeros(n, bool)
    idx = np.flatnonzero(valid)
    x = torch.from_numpy(soa[:, idx].astype(np.float64)).to(dtype).requires_grad_(upstream is not None)
    f = forward(x, camv, W, H, t)
    out = {"valid": valid, "ambiguous": amb}
    for k in ("color", "raw", "opacity", "conic", "center", "view", "ndc", "det"):
        a = f[k].detach().numpy()
        full = np.full(a.shape[:-1] + (n,), np.nan, a.dtype)
        full[..., idx] = a
        out[k] = full
    if upstream is None:
        return out
    rec = torch.cat([f["color"], f["opacity"][None], f["conic"], f["center"]])      # (10, m)
    up = torch.from_numpy(np.asarray(upstream, np.float64)[:, idx]).to(dtype)
    grad, absg = np.zeros((narrays, n), np.float64), np.zeros((narrays, n), np.float64)
    for c in range(10):
        if not up[c].any():
            continue
        (g,) = torch.autograd.grad((rec[c] * up[c]).sum(), x, retain_graph=True)
        g = g.numpy().astype(np.float64)
        grad[:, idx] += g
        absg[:, idx] += np.abs(g)
    out["grad"], out["abs"] = grad, absg
    return out


def scale(absg, narrays):
    """A as a (narrays, n) array: every array of a group carries the group's scale."""
    A = np.zeros_like(absg)
    for rows in groups(narrays).values():
        A[rows] = absg[rows].max(0, keepdims=True)
    return A


def error_over_scale(got, ref_grad, A):
    """The largest |got - ref| / A over the entries with A > 0 (0.0 when there are none)."""
    pos = A > 0
    if not pos.any():
        return 0.0
    return float((np.abs(np.asarray(got, np.float64) - ref_grad)[pos] / A[pos]).max())


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
            f = forward(torch.from_numpy(cpy), camv, W, H, t)
        rec = torch.cat([f["color"], f["opacity"][None], f["conic"], f["center"]]).numpy()[:, 0]
        vals.append(rec * np.asarray(upstream, np.float64)[:, i])
    return float((vals[0] - vals[1]).sum()) / (2 * h)     # differenced per component, then summed


# ---------------------------------------------------------------- the cases the GPU tests use

# name: scene, camera (test_gpu_parity.cam_for's arguments), W, H, time, the first `first`
# Gaussians only.  The smallest shapes at which the kernel can still go wrong: one partial
# workgroup with identity quaternions (dense); un-normalised random quaternions (rot); 7.8
# workgroups, hundreds of Gaussians off screen (sparse_a, sparse_b), a camera inside the cloud
# with >= 100 Gaussians that fail the validity tests (sparse_in); 48 SH planes (sh3);
# the temporal arrays (4d); a block stride (64, 320) that differs from n, and a second
# workgroup of one lane (n1, n257).
CASES = {
    "dense": dict(scene="dense", cam={}, W=70, H=52),
    "rot": dict(scene="rot", cam={}, W=70, H=52),
    "sparse_a": dict(scene="sparse", cam=0, W=160, H=120),
    "sparse_b": dict(scene="sparse", cam=3, W=160, H=120),
    "sparse_in": dict(scene="sparse", cam=dict(pos=(0.3, 0.1, 0.2), look=(0.2, 0, -1.0), fov=70), W=160, H=120),
    "sh3": dict(scene="sh3", cam=0, W=160, H=120),
    "4d": dict(scene="4d", cam={}, W=160, H=120, time=0.3),
    "n1": dict(scene="rot", cam={}, W=70, H=52, first=1),
    "n257": dict(scene="rot257", cam={}, W=70, H=52, first=257),
}
SEEDS = {name: 100 + k for k, name in enumerate(CASES)}

_scenes, _refs = {}, {}


def scenes(gsr, tmp_path_factory):
    if not _scenes:
        from test_gpu_contrib import dense_soa
        d = tmp_path_factory.mktemp("project_scenes")
        p = str(d / "sparse.ply")
        gsr.write_synthetic_ply(p, 2000, 1)
        p4 = str(d / "scene4d.ply")
        gsr.write_synthetic_ply4d(p4, 1500, 5)
        rot = dense_soa()
        rot[7:11] = np.random.default_rng(41).standard_normal((4, rot.shape[1])).astype(np.float32)
        # 257 Gaussians: the dense scene's 200 and 57 of them again, moved a little
        rot257 = np.concatenate([rot, rot[:, :57]], axis=1)
        rot257[0:3, 200:] += np.float32(0.05)
        _scenes.update({"dense": dense_soa(), "rot": rot, "rot257": rot257, "sparse": gsr.read_ply(p),
                        "sh3": gsr.read_ply(p, sh3=True), "4d": gsr.read_ply(p4, four_d=True)})
    return _scenes


def camera(gsr, case):
    from test_gpu_parity import CAMS, cam_for
    c = CASES[case]
    kw = CAMS[c["cam"]] if isinstance(c["cam"], int) else c["cam"]
    return cam_for(gsr, c["W"], c["H"], **kw)


def case_soa(gsr, tmp_path_factory, case):
    c = CASES[case]
    soa = scenes(gsr, tmp_path_factory)[c["scene"]]
    return np.ascontiguousarray(soa[:, :c["first"]]) if "first" in c else soa


def reference(gsr, tmp_path_factory, case):
    """The float64 reference of one case, computed once and left unchanged: evaluate()'s dict
    plus "soa", "camv", "upstream" (10, n) float32, standard normal on ALL n Gaussians and then
    zeroed at the ambiguous ones, and "A" (narrays, n)."""
    if case not in _refs:
        c = CASES[case]
        soa = case_soa(gsr, tmp_path_factory, case)
        camv = camera_values(gsr, camera(gsr, case))
        n = soa.shape[1]
        up = np.random.default_rng(SEEDS[case]).standard_normal((10, n)).astype(np.float32)
        first = evaluate(soa, camv, c["W"], c["H"], c.get("time", 0.0))
        up[:, first["ambiguous"]] = 0.0
        under = np.zeros(n, bool)
        if soa.shape[0] == 49:
            # float32's exp underflows where the temporal factor nears 1e-38: no relative scale
            # can hold for what is multiplied by it, so these Gaussians (culled in time, far
            # below the temporal cull's 0.9e-3) get no upstream on their opacity
            s64 = soa.astype(np.float64)
            under = np.exp(-((c["time"] - s64[38]) / s64[39]) ** 2) < TFAC_MIN
            up[3, under] = 0.0
        res = evaluate(soa, camv, c["W"], c["H"], c.get("time", 0.0), upstream=up, valid=first["valid"])
        res["ambiguous"] = first["ambiguous"]
        res["underflow"] = under
        res.update(soa=soa, camv=camv, upstream=up, A=scale(res["abs"], soa.shape[0]))
        for v in res.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _refs[case] = res
    return _refs[case]


def ambiguous_share(res):
    return float(res["ambiguous"].sum()) / max(int(res["valid"].sum()), 1)
