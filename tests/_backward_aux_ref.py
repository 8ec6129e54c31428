"""Reference of gsr_render_backward_aux (include/gsr.h) — TEST INFRASTRUCTURE.

tests/_backward_ref.py's numpy evaluation extended to

    L = sum over pixels of g_rgb . image + g_A alpha + g_D depth + sum_f g_f feat_f

in float64 (the yardstick) or float32 (what single precision alone costs).  The records gain
"z" (1, n), the oracle's -view z as float64 copies of its float32 (what gsr_render_aux
composites into its depth plane), and "feat" (nfeat, n), seeded standard-normal float32
feature values.  The boxes, the blend, the ambiguity mask and MASK_SHARE_CAP are
_backward_ref's; the mask depends on the forward decisions only, so it does not move with the
upstream gradients.
"""
from __future__ import annotations

import numpy as np

import _backward_ref as br

BASE = br.KINDS                       # colour 3, opacity 1, conic 4, centre 2
MASK_SHARE_CAP = br.MASK_SHARE_CAP


def kinds(nfeat):
    """(name, components) of every output: _backward_ref.KINDS, then z and the features."""
    return BASE + (("z", 1),) + ((("feat", nfeat),) if nfeat else ())


def rows(nfeat):
    """name -> rows of the (11 + nfeat, n) block the GPU tests hold every output in."""
    out, at = {}, 0
    for name, c in kinds(nfeat):
        out[name] = slice(at, at + c)
        at += c
    return out


def features(n, nfeat, seed):
    """(nfeat, n) float32, standard normal: mixed signs."""
    return np.random.default_rng(1000 + seed).standard_normal((nfeat, n)).astype(np.float32)


def records(orc, soa, cam, W, H, k=3.0, feat=None):
    """_backward_ref.records plus "z" and "feat"."""
    rec = br.records(orc, soa, cam, W, H, k)
    spl = orc.preprocess(soa, cam, W, H, k)
    rec["z"] = (-spl["view"][:, 2]).astype(np.float32).astype(np.float64)[None].copy()      # (1, n)
    rec["feat"] = np.zeros((0, rec["n"])) if feat is None else np.asarray(feat, np.float32).astype(np.float64)
    return rec


def evaluate(rec, W, H, g_image=None, g_alpha=None, g_depth=None, g_feat=None, tiling=None, dtype=np.float64,
             zero_masked=True, region=None, grads=True):
    """The forward blend with its depth and feature planes and (grads=True) the gradients.

    g_image (3, H, W) / g_alpha (H, W) / g_depth (H, W) / g_feat (nfeat, H, W), None = zeros.
    zero_masked: the upstream gradients are zeroed at ambiguous pixels first (the returned
    "g_*" are what was used).  region (x0, x1, y0, y1): only these pixels are evaluated.
    Returns image, alpha, depth, feat, takes, count, mask, L (Lp: per pixel) and, per kind of
    kinds(nfeat), the gradient planes (c, n) under its name and their scale planes (the sums of
    the absolute values of the terms, float64) under "A_" + name."""
    f = np.dtype(dtype).type
    n = rec["n"]
    nfeat = rec["feat"].shape[0]
    cw, ch = br.cover(W, H, tiling)
    gi = np.zeros((3, H, W), dtype) if g_image is None else np.array(g_image, dtype).reshape(3, H, W)
    ga = np.zeros((H, W), dtype) if g_alpha is None else np.array(g_alpha, dtype).reshape(H, W)
    gd = np.zeros((H, W), dtype) if g_depth is None else np.array(g_depth, dtype).reshape(H, W)
    gf = np.zeros((nfeat, H, W), dtype) if g_feat is None else np.array(g_feat, dtype).reshape(nfeat, H, W)
    col, opa = rec["color"].astype(dtype), rec["opacity"].astype(dtype)[0]
    con, cen = rec["conic"].astype(dtype), rec["center"].astype(dtype)
    zz, ft = rec["z"].astype(dtype)[0], rec["feat"].astype(dtype)
    xs, ys = np.arange(W, dtype=dtype), np.arange(H, dtype=dtype)

    T = np.ones((H, W), dtype)
    image, alpha_acc = np.zeros((3, H, W), dtype), np.zeros((H, W), dtype)
    depth, feat = np.zeros((H, W), dtype), np.zeros((nfeat, H, W), dtype)
    takes, mask = np.zeros((H, W), np.int64), np.zeros((H, W), bool)
    count = np.zeros(n, np.int64)
    steps = []
    for i, sy, sx in br._boxes(rec, cw, ch, region):
        dx = (xs[sx] - cen[0, i])[None, :] + np.zeros((sy.stop - sy.start, 1), dtype)
        dy = (ys[sy] - cen[1, i])[:, None] + np.zeros((1, sx.stop - sx.start), dtype)
        a, b, c, e = con[:, i]
        md2 = dx * (a * dx + b * dy) + dy * (c * dx + e * dy)
        E = np.exp(f(-0.5) * md2)
        oe = opa[i] * E
        al = np.minimum(oe, f(br.ALPHA_MAX))
        Tb = T[sy, sx].copy()
        live = ~(Tb < f(br.T_MIN))
        take = live & ~(al < f(br.ALPHA_MIN))
        oe64 = oe.astype(np.float64)
        ring = ((np.abs(oe64 - br.ALPHA_MIN) <= br.RING_ALPHA * br.ALPHA_MIN)
                | (np.abs(oe64 - br.ALPHA_MAX) <= br.RING_ALPHA * br.ALPHA_MAX))
        mask[sy, sx] |= (live & ring) | (np.abs(Tb.astype(np.float64) - br.T_MIN) <= br.RING_T * br.T_MIN)
        w = np.where(take, al * Tb, f(0))
        for chn in range(3):
            image[chn, sy, sx] += col[chn, i] * w
        alpha_acc[sy, sx] += w
        depth[sy, sx] += zz[i] * w
        for j in range(nfeat):
            feat[j, sy, sx] += ft[j, i] * w
        T[sy, sx] = np.where(take, Tb * (f(1) - al), Tb)
        takes[sy, sx] += take
        count[i] = take.sum()
        steps.append((i, sy, sx, dx, dy, E, oe, al, Tb, take, w))
    if zero_masked:
        gi = np.where(mask[None], f(0), gi)
        ga = np.where(mask, f(0), ga)
        gd = np.where(mask, f(0), gd)
        gf = np.where(mask[None], f(0), gf)
    Lp = (gi * image).sum(0) + ga * alpha_acc + gd * depth + (gf * feat).sum(0)
    out = {"image": image, "alpha": alpha_acc, "depth": depth, "feat_planes": feat, "takes": takes, "mask": mask,
           "g_image": gi, "g_alpha": ga, "g_depth": gd, "g_feat": gf, "count": count, "Lp": Lp, "L": float(Lp.sum())}
    if not grads:
        return out

    def u_of(i, sy, sx):
        u = gi[0, sy, sx] * col[0, i] + gi[1, sy, sx] * col[1, i] + gi[2, sy, sx] * col[2, i] + ga[sy, sx]
        u = u + gd[sy, sx] * zz[i]
        for j in range(nfeat):
            u = u + gf[j, sy, sx] * ft[j, i]
        return u

    P, M = np.zeros((H, W), dtype), np.zeros((H, W), dtype)
    for i, sy, sx, dx, dy, E, oe, al, Tb, take, w in steps:
        u = u_of(i, sy, sx)
        P[sy, sx] += u * w
        M[sy, sx] += np.abs(u) * w
    G = P
    P = np.zeros((H, W), dtype)
    for name, c in kinds(nfeat):
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
        out["z"][0, i] += (gd[sy, sx] * w).sum()
        out["A_z"][0, i] += (np.abs(gd[sy, sx]) * w).astype(np.float64).sum()
        for j in range(nfeat):
            out["feat"][j, i] += (gf[j, sy, sx] * w).sum()
            out["A_feat"][j, i] += (np.abs(gf[j, sy, sx]) * w).astype(np.float64).sum()
        free = take & ~(oe > f(br.ALPHA_MAX))
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


def finite_difference(rec, W, H, g, kind, comp, i, tiling=None, rel=1e-6):
    """Central difference of L with respect to component `comp` of `kind` (a record array, "z"
    or "feat") of Gaussian i, over the splat's box only; g: the four upstream gradients."""
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
        Ls.append(evaluate(r, W, H, *g, tiling=tiling, zero_masked=False, region=region, grads=False)["Lp"])
    # differenced per pixel, so the other splats' shares of L cancel before anything is summed
    return float((Ls[0] - Ls[1]).sum()) / (2 * h)


def error_over_scale(got, ref, nfeat):
    """The largest |got - ref| / A over every kind, component and Gaussian with A > 0, and
    whether every entry with A = 0 is exactly 0 in `got`."""
    worst, clean = 0.0, True
    for name, _ in kinds(nfeat):
        A = ref["A_" + name]
        d = np.abs(np.asarray(got[name], np.float64) - ref[name].astype(np.float64))
        pos = A > 0
        if pos.any():
            worst = max(worst, float((d[pos] / A[pos]).max()))
        clean = clean and not np.asarray(got[name])[~pos].any()
    return worst, clean


# ---------------------------------------------------------------- the runs the GPU tests compare

def spec(seed, image=True, alpha=True, depth=True, nfeat=0, feat_up=None):
    """One run's upstream: which gradients are given, how many features the scene carries and
    whether their planes have an upstream gradient (default: they do)."""
    return (seed, image, alpha, depth, nfeat, bool(nfeat) if feat_up is None else feat_up)


def upstream(W, H, sp):
    """(g_image, g_alpha, g_depth, g_feat) float32, standard normal; None where not given."""
    seed, image, alpha, depth, nfeat, feat_up = sp
    rng = np.random.default_rng(seed)
    gi = rng.standard_normal((3, H, W)).astype(np.float32)
    ga = rng.standard_normal((H, W)).astype(np.float32)
    gd = rng.standard_normal((H, W)).astype(np.float32)
    gf = rng.standard_normal((max(nfeat, 1), H, W)).astype(np.float32)[:nfeat]
    return (gi if image else None, ga if alpha else None, gd if depth else None, gf if feat_up else None)


ALL4, ALL8 = spec(21, nfeat=4), spec(25, nfeat=8)
# (case of _backward_ref.CASES, upstream) of every GPU comparison: the smallest shapes at which
# the kernel can go wrong (70 x 52: partial tiles and blocks; 160 x 120: thousands of short
# lists; faint: lists of 47 batches), every padding of the feature count (1, 2, 3 -> 4; 5 -> 8,
# packed), each channel alone and all together
RUNS_AUX = [
    ("dense", spec(20, image=False, alpha=False)),                      # depth only
    ("dense", spec(22, image=False, alpha=False, depth=False, nfeat=1)),  # one feature only
    ("dense", ALL4),
    ("dense", spec(23, nfeat=5)),
    ("dense", spec(24, nfeat=8)),
    ("dense99", spec(26, nfeat=3)),
    ("dense_partial", spec(27, nfeat=2)),
    ("sparse_a", ALL8), ("sparse_b", spec(28, nfeat=8)),
    ("4d", spec(29, alpha=False)),
    ("faint", spec(30, image=False, alpha=False, nfeat=8)),
    ("tilted_k8", spec(31, nfeat=4)),
    ("overflow", spec(32, nfeat=4)),
]

_refs = {}


def reference(gsr, orc, tmp_path_factory, case, sp=ALL4, grads=True):
    """The float64 reference of one run, computed once and left unchanged: evaluate()'s dict
    plus "rec", "soa" and "features" ((nfeat, n) float32, None without features); upstream
    gradients that were not given read None."""
    key = (case, sp, grads)
    if key not in _refs:
        c = br.CASES[case]
        soa = br.scenes(gsr, orc, tmp_path_factory)[c["scene"]]
        if "time" in c:
            soa = orc.temporal(soa, c["time"])
        nfeat = sp[4]
        feats = features(soa.shape[1], nfeat, sp[0]) if nfeat else None
        rec = records(orc, soa, br.camera(gsr, case), c["W"], c["H"], c.get("k", 3.0), feats)
        g = list(upstream(c["W"], c["H"], sp))
        if "region" in c:
            x0, x1, y0, y1 = c["region"]
            keep = np.zeros((c["H"], c["W"]), bool)
            keep[y0:y1 + 1, x0:x1 + 1] = True
            g = [None if a is None else np.where(keep, a, np.float32(0)) for a in g]
        res = evaluate(rec, c["W"], c["H"], *g, tiling=c.get("tiling"), region=c.get("region"), grads=grads)
        for name, a in zip(("g_image", "g_alpha", "g_depth", "g_feat"), g):
            if a is None:
                res[name] = None
        res["rec"], res["soa"], res["features"], res["nfeat"] = rec, soa, feats, nfeat
        for v in list(res.values()) + list(rec.values()):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _refs[key] = res
    return _refs[key]


def upstream_of(r):
    """The four upstream gradients a reference used (zero at ambiguous pixels), None = not given."""
    return r["g_image"], r["g_alpha"], r["g_depth"], r["g_feat"]
