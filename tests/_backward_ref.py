"""Reference of gsr_render_backward (include/gsr.h) — TEST INFRASTRUCTURE.

A numpy evaluation of the header's formulas, in float64 (the yardstick) or float32 (to
measure what single precision alone costs).  Its inputs come from the unmodified oracle:
`_oracle.preprocess` records (status 2 only) in `_oracle.expected_depth_order`, with the
oracle's aabb as the box.  The blend it differentiates is the oracle's blend_step.

Decisions that floating point could take either way are not compared: a pixel is AMBIGUOUS
when, at any splat it visits while T >= 1e-3, o E lies within a relative 1e-4 of 1e-3 or of
0.99, or T within a relative 1e-3 of 1e-3.  fp32 errors in alpha are about 3e-6 relative and
in T at most about 2e-5 after hundreds of factors, so outside the mask fp32 and fp64 take the
same decisions.  Tests zero the upstream gradient at masked pixels on both sides.
"""
from __future__ import annotations

import numpy as np

ALPHA_MIN, ALPHA_MAX, T_MIN = 1e-3, 0.99, 1e-3
RING_ALPHA, RING_T = 1e-4, 1e-3
MASK_SHARE_CAP = 0.02

KINDS = (("color", 3), ("opacity", 1), ("conic", 4), ("center", 2))


def records(orc, soa, cam, W, H, k=3.0):
    """The frame's splat records as float64 parameter arrays (exact copies of the oracle's
    float32 / integer values) and the visible Gaussians in depth order."""
    spl = orc.preprocess(soa, cam, W, H, k)
    nvis = int((spl["status"] == 2).sum())
    order = (orc.expected_depth_order(spl)[:nvis] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    return {
        "n": spl.shape[0],
        "order": order,
        "aabb": spl["aabb"].astype(np.int64),
        "color": spl["color"].astype(np.float64).T.copy(),          # (3, n)
        "opacity": spl["opacity"].astype(np.float64)[None].copy(),  # (1, n)
        "conic": spl["inv_covar"].astype(np.float64).T.copy(),      # (4, n)
        "center": np.stack([spl["px_x"], spl["px_y"]]).astype(np.float64),   # (2, n)
    }


def cover(W, H, tiling=None):
    nx, ny, ws, hs = tiling if tiling else (1, 1, W, H)
    return min(nx * ws, W), min(ny * hs, H)


def _boxes(rec, cw, ch, region):
    """[(gaussian, y slice, x slice)] of the visible splats whose box meets the region."""
    rx0, rx1, ry0, ry1 = region if region else (0, cw - 1, 0, ch - 1)
    rx0, ry0, rx1, ry1 = max(rx0, 0), max(ry0, 0), min(rx1, cw - 1), min(ry1, ch - 1)
    out = []
    for i in rec["order"]:
        x0, y0, x1, y1 = rec["aabb"][i]
        x0, y0, x1, y1 = max(x0, rx0), max(y0, ry0), min(x1, rx1), min(y1, ry1)
        if x0 <= x1 and y0 <= y1:
            out.append((int(i), slice(y0, y1 + 1), slice(x0, x1 + 1)))
    return out


def evaluate(rec, W, H, g_image=None, g_alpha=None, tiling=None, dtype=np.float64, zero_masked=True,
             region=None, grads=True):
    """The forward blend and (grads=True) its gradients.

    g_image (3, H, W) / g_alpha (H, W), None = zeros.  zero_masked: the upstream gradient is
    zeroed at ambiguous pixels first (the returned "g_image" / "g_alpha" are what was used).
    region (x0, x1, y0, y1): only these pixels are evaluated (finite differences).
    Returns image, alpha, takes, count (pixels per Gaussian), mask, L = sum g . image + g_A alpha (Lp: per pixel), and per kind of KINDS the
    gradient planes (c, n) under its name and their scale planes under "A_" + name."""
    f = np.dtype(dtype).type
    n = rec["n"]
    cw, ch = cover(W, H, tiling)
    gi = np.zeros((3, H, W), dtype) if g_image is None else np.array(g_image, dtype).reshape(3, H, W)
    ga = np.zeros((H, W), dtype) if g_alpha is None else np.array(g_alpha, dtype).reshape(H, W)
    col, opa = rec["color"].astype(dtype), rec["opacity"].astype(dtype)[0]
    con, cen = rec["conic"].astype(dtype), rec["center"].astype(dtype)
    xs, ys = np.arange(W, dtype=dtype), np.arange(H, dtype=dtype)

    T = np.ones((H, W), dtype)
    image, alpha_acc = np.zeros((3, H, W), dtype), np.zeros((H, W), dtype)
    takes, mask = np.zeros((H, W), np.int64), np.zeros((H, W), bool)
    count = np.zeros(n, np.int64)
    steps = []
    for i, sy, sx in _boxes(rec, cw, ch, region):
        dx = (xs[sx] - cen[0, i])[None, :] + np.zeros((sy.stop - sy.start, 1), dtype)
        dy = (ys[sy] - cen[1, i])[:, None] + np.zeros((1, sx.stop - sx.start), dtype)
        a, b, c, e = con[:, i]
        md2 = dx * (a * dx + b * dy) + dy * (c * dx + e * dy)
        E = np.exp(f(-0.5) * md2)
        oe = opa[i] * E
        al = np.minimum(oe, f(ALPHA_MAX))
        Tb = T[sy, sx].copy()
        live = ~(Tb < f(T_MIN))
        take = live & ~(al < f(ALPHA_MIN))
        oe64 = oe.astype(np.float64)
        ring = (np.abs(oe64 - ALPHA_MIN) <= RING_ALPHA * ALPHA_MIN) | (np.abs(oe64 - ALPHA_MAX) <= RING_ALPHA * ALPHA_MAX)
        mask[sy, sx] |= (live & ring) | (np.abs(Tb.astype(np.float64) - T_MIN) <= RING_T * T_MIN)
        w = np.where(take, al * Tb, f(0))
        for chn in range(3):
            image[chn, sy, sx] += col[chn, i] * w
        alpha_acc[sy, sx] += w
        T[sy, sx] = np.where(take, Tb * (f(1) - al), Tb)
        takes[sy, sx] += take
        count[i] = take.sum()
        steps.append((i, sy, sx, dx, dy, E, oe, al, Tb, take, w))
    if zero_masked:
        gi = np.where(mask[None], f(0), gi)
        ga = np.where(mask, f(0), ga)
    Lp = (gi * image).sum(0) + ga * alpha_acc      # the pixels' shares of L
    out = {"image": image, "alpha": alpha_acc, "takes": takes, "mask": mask, "g_image": gi, "g_alpha": ga,
           "count": count, "Lp": Lp, "L": float(Lp.sum())}
    if not grads:
        return out

    # G = P_last and M = sum |u| alpha T, then the same accumulation of P again
    def u_of(i, sy, sx):
        return gi[0, sy, sx] * col[0, i] + gi[1, sy, sx] * col[1, i] + gi[2, sy, sx] * col[2, i] + ga[sy, sx]

    P, M = np.zeros((H, W), dtype), np.zeros((H, W), dtype)
    for i, sy, sx, dx, dy, E, oe, al, Tb, take, w in steps:
        u = u_of(i, sy, sx)
        P[sy, sx] += u * w
        M[sy, sx] += np.abs(u) * w
    G = P
    P = np.zeros((H, W), dtype)
    for name, c in KINDS:
        out[name] = np.zeros((c, n), dtype)
        out["A_" + name] = np.zeros((c, n), np.float64)
    for i, sy, sx, dx, dy, E, oe, al, Tb, take, w in steps:
        if not take.any():
            continue
        u = u_of(i, sy, sx)
        P[sy, sx] += u * w
        for chn in range(3):
            out["color"][chn, i] += (gi[chn, sy, sx] * w).sum()
            out["A_color"][chn, i] += (np.abs(gi[chn, sy, sx]) * w).astype(np.float64).sum()
        free = take & ~(oe > f(ALPHA_MAX))
        da = np.where(free, Tb * u - (G[sy, sx] - P[sy, sx]) / (f(1) - al), f(0))
        sa = np.where(free, Tb * np.abs(u) + M[sy, sx] / (f(1) - al), f(0)).astype(np.float64)
        a, b, c, e = con[:, i]
        h = f(-0.5) * oe          # d alpha / d md2
        parts = {
            "opacity": [E],
            "conic": [h * dx * dx, h * dx * dy, h * dx * dy, h * dy * dy],
            "center": [-h * (f(2) * a * dx + (b + c) * dy), -h * ((b + c) * dx + f(2) * e * dy)],
        }
        for name, ds in parts.items():
            for j, d in enumerate(ds):
                out[name][j, i] += (da * d).sum()
                out["A_" + name][j, i] += (sa * np.abs(d).astype(np.float64)).sum()
    return out


def mask_share(res):
    """Masked share of the covered pixels (those that composite anything or are masked)."""
    covered = (res["takes"] > 0) | res["mask"]
    return float(res["mask"].sum()) / max(int(covered.sum()), 1)


def finite_difference(rec, W, H, g_image, g_alpha, kind, comp, i, tiling=None, rel=1e-6):
    """Central difference of L with respect to component `comp` of `kind` of Gaussian i, over
    the splat's box only (no other pixel depends on it)."""
    x0, y0, x1, y1 = rec["aabb"][i]
    region = (int(x0), int(x1), int(y0), int(y1))
    v = rec[kind][comp, i]
    floor = np.abs(rec["conic"][:, i]).max() if kind == "conic" else 1.0
    h = rel * max(abs(v), floor)
    Ls = []
    for s in (+1, -1):
        r = dict(rec)
        r[kind] = rec[kind].copy()
        r[kind][comp, i] = v + s * h
        Ls.append(evaluate(r, W, H, g_image, g_alpha, tiling, zero_masked=False, region=region, grads=False)["Lp"])
    # differenced per pixel, so the other splats' shares of L cancel before anything is summed
    return float((Ls[0] - Ls[1]).sum()) / (2 * h)


def error_over_scale(got, ref):
    """The largest |got - ref| / A over every kind, component and Gaussian with A > 0, and
    whether every entry with A = 0 is exactly 0 in `got` (a difference from the prefill)."""
    worst, clean = 0.0, True
    for name, _ in KINDS:
        if name not in got:
            continue
        A = ref["A_" + name]
        d = np.abs(np.asarray(got[name], np.float64) - ref[name].astype(np.float64))
        pos = A > 0
        if pos.any():
            worst = max(worst, float((d[pos] / A[pos]).max()))
        clean = clean and not np.asarray(got[name])[~pos].any()
    return worst, clean


# ---------------------------------------------------------------- the cases the GPU tests use

def overflow_soa():
    """tests/test_gpu_contrib.py's overflow scene: 3000 huge, faint splats."""
    n = 3000
    rng = np.random.default_rng(9)
    soa = np.zeros((38, n), np.float32)
    soa[0] = rng.uniform(-0.2, 0.2, n); soa[1] = rng.uniform(-0.2, 0.2, n); soa[2] = rng.uniform(-0.2, 0.2, n)
    soa[3] = rng.uniform(0.01, 0.05, n)
    soa[4:7] = rng.uniform(1.0, 2.0, (3, n))
    soa[7] = 1.0
    soa[11:38] = rng.normal(0, 0.3, (27, n))
    return soa


def upstream(W, H, seed, ones=False, image=True, alpha=True):
    """(g_image, g_alpha) float32: standard normal (mixed signs) or ones; None where not given."""
    rng = np.random.default_rng(seed)
    gi = np.ones((3, H, W), np.float32) if ones else rng.standard_normal((3, H, W)).astype(np.float32)
    ga = np.ones((H, W), np.float32) if ones else rng.standard_normal((H, W)).astype(np.float32)
    return (gi if image else None), (ga if alpha else None)


# name: scene, camera (test_gpu_parity.cam_for's arguments), W, H, tiling, k, time.  The
# smallest shapes at which the kernel can still go wrong: partial tiles and 8x8 blocks, W no
# multiple of 8, lists of four batches (dense), early saturation (dense99), a tiling that
# covers 60 x 40 of 70 x 52, thousands of short lists (sparse), lists of 47 batches (faint).
CASES = {
    "dense": dict(scene="dense", cam={}, W=70, H=52),
    "dense99": dict(scene="dense99", cam={}, W=70, H=52),
    "dense_partial": dict(scene="dense", cam={}, W=70, H=52, tiling=(3, 2, 20, 20)),
    "sparse_a": dict(scene="sparse", cam=0, W=160, H=120),
    "sparse_b": dict(scene="sparse", cam=3, W=160, H=120),
    "4d": dict(scene="4d", cam={}, W=160, H=120, time=0.3),
    # the same scene from far away with a box factor of 0.5: 25 pixels of two tiles composite
    # lists of 3000 records (47 batches), up to 483 takes per pixel, with no ambiguous pixel
    "faint": dict(scene="overflow", cam=dict(pos=(0, 0, 90)), W=160, H=120, k=0.5),
    # tests/test_gpu_contrib.py's overflowing frame.  OUTSIDE the mask-share condition, by
    # construction: a frame overflows the smallest pair buffer (2^20 pairs) only if its 3000
    # boxes cover 350 tiles each, so every pixel composites hundreds to thousands of faint
    # splats and saturates, and a transmittance that falls in steps of about 3 % lands in the
    # ambiguity ring of T at 5-10 % of such pixels, whatever the camera or the box factor
    # (measured 4-18 %; this frame: 15 %).  The float32 oracle's own image is 1.6e-6 off here
    # after 1700 takes, too.  So the upstream gradient of this case is non-zero only in
    # REGION (12 x 10 pixels over a corner of four tiles), which keeps the reference to a few
    # seconds; its ambiguous pixels are zeroed like any others.
    "overflow": dict(scene="overflow", cam={}, W=640, H=480, region=(314, 325, 235, 244)),
    # _wide_scenes' tilted scene: random quaternions and scales of 0.02 - 0.5, so the conics
    # have off-diagonal terms of their own (the dense scenes' quaternion is the identity) and
    # the ellipses cross many blocks at an angle; with k = 8 the boxes cover the frame
    "tilted": dict(scene="tilted", cam={}, W=70, H=52),
    "tilted_k8": dict(scene="tilted", cam=1, W=90, H=70, k=8.0),
}
# (case, upstream gradient: seed, ones, image given, alpha given) of every GPU comparison
RUNS = [
    ("dense", (5, False, True, True)), ("dense", (0, True, True, True)),
    ("dense", (6, False, False, True)), ("dense", (7, False, True, False)),
    ("sparse_a", (8, False, True, True)), ("sparse_a", (0, True, True, True)),
    ("sparse_b", (9, False, True, True)), ("sparse_b", (0, True, True, True)),
    ("dense99", (10, False, True, True)), ("dense_partial", (11, False, True, True)),
    ("4d", (12, False, True, True)), ("faint", (13, False, True, True)), ("overflow", (14, False, True, True)),
    ("tilted", (15, False, True, True)), ("tilted_k8", (16, False, True, True)),
]

_scenes, _refs = {}, {}


def scenes(gsr, orc, tmp_path_factory):
    """name -> the scene's arrays ((38, n), or (49, n) for "4d")."""
    if not _scenes:
        from test_gpu_contrib import dense_soa
        from _wide_scenes import scene as wide_scene
        d = tmp_path_factory.mktemp("backward_scenes")
        p = str(d / "sparse.ply")
        gsr.write_synthetic_ply(p, 2000, 1)
        p4 = str(d / "scene4d.ply")
        gsr.write_synthetic_ply4d(p4, 1500, 5)
        d99 = dense_soa()
        d99[3] = 0.99
        _scenes.update({"dense": dense_soa(), "dense99": d99, "sparse": gsr.read_ply(p),
                        "4d": gsr.read_ply(p4, four_d=True), "overflow": overflow_soa(),
                        "tilted": wide_scene("tilted")})
    return _scenes


def camera(gsr, case):
    from test_gpu_parity import CAMS, cam_for
    c = CASES[case]
    kw = CAMS[c["cam"]] if isinstance(c["cam"], int) else c["cam"]
    return cam_for(gsr, c["W"], c["H"], **kw)


def reference(gsr, orc, tmp_path_factory, case, g=(5, False, True, True)):
    """The float64 reference of one run, computed once and left unchanged: evaluate()'s
    dict plus "rec" (the records) and "soa" (the (38, n) scene the oracle renders)."""
    key = (case, g)
    if key not in _refs:
        c = CASES[case]
        soa = scenes(gsr, orc, tmp_path_factory)[c["scene"]]
        if "time" in c:
            soa = orc.temporal(soa, c["time"])
        rec = records(orc, soa, camera(gsr, case), c["W"], c["H"], c.get("k", 3.0))
        gi, ga = upstream(c["W"], c["H"], *g)
        if "region" in c:
            x0, x1, y0, y1 = c["region"]
            keep = np.zeros((c["H"], c["W"]), bool)
            keep[y0:y1 + 1, x0:x1 + 1] = True
            gi, ga = [None if a is None else np.where(keep, a, np.float32(0)) for a in (gi, ga)]
        res = evaluate(rec, c["W"], c["H"], gi, ga, c.get("tiling"), region=c.get("region"))
        if gi is None:
            res["g_image"] = None
        if ga is None:
            res["g_alpha"] = None
        res["rec"], res["soa"] = rec, soa
        for v in res.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _refs[key] = res
    return _refs[key]
