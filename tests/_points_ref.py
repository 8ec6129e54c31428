"""Numpy twins of the scene initialisation (include/gsr.h "scene initialisation"): the exact
3-nearest-neighbour statistic of gsr_points_knn_dist2 as a chunked float32 brute force, and the
fill of gsr_scene_from_points.  Also the clouds the CPU and GPU tests share."""
import numpy as np

SH_C0 = np.float32(0.28209479177387814)
LEAF, FAN, BOUNDS_CHUNK, SORT_TILE = 64, 64, 2048, 4096   # gsr_internal.h kKnn*, kSortTile
F32 = np.float32


def valid_mask(xyz):
    return np.isfinite(np.asarray(xyz, F32)).all(axis=1)


def knn_rows(xyz, rows, chunk=1024):
    """mean2 of the points `rows` (indices) of the float32 cloud xyz [n, 3] by the rule: every
    operation float32 with its own rounding, d2 = ((dx*dx) + (dy*dy)) + (dz*dz), self excluded
    by index, invalid points nobody's neighbour and +0 themselves."""
    xyz = np.ascontiguousarray(xyz, F32)
    rows = np.asarray(rows, np.int64)
    ok = valid_mask(xyz)
    vidx = np.flatnonzero(ok)
    m = vidx.size
    k = min(3, m - 1)
    out = np.zeros(rows.size, F32)
    if k <= 0:
        return out
    P = xyz[vidx]
    px, py, pz = P[:, 0][None, :], P[:, 1][None, :], P[:, 2][None, :]
    pos_of = np.full(xyz.shape[0], -1, np.int64)
    pos_of[vidx] = np.arange(m)
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(0, rows.size, chunk):
            r = rows[s:s + chunk]
            sel = np.flatnonzero(ok[r])
            if sel.size == 0:
                continue
            q = xyz[r[sel]]
            dx = px - q[:, 0][:, None]
            dy = py - q[:, 1][:, None]
            dz = pz - q[:, 2][:, None]
            d2 = ((dx * dx) + (dy * dy)) + (dz * dz)
            assert d2.dtype == F32
            d2[np.arange(sel.size), pos_of[r[sel]]] = np.inf     # self, by index
            # a genuine +inf distance and the masked self are the same value: with k <= m - 1
            # real candidates the k smallest values are unchanged by the mask
            b = np.sort(np.partition(d2, k - 1, axis=1)[:, :k], axis=1)
            if k == 3:
                v = ((b[:, 0] + b[:, 1]) + b[:, 2]) / F32(3.0)
            elif k == 2:
                v = (b[:, 0] + b[:, 1]) / F32(2.0)
            else:
                v = b[:, 0]
            out[s + sel] = v.astype(F32)
    return out


def knn_dist2(xyz, chunk=1024):
    """(mean2 [n], the number of invalid points)."""
    xyz = np.ascontiguousarray(xyz, F32).reshape(-1, 3)
    n = xyz.shape[0]
    return knn_rows(xyz, np.arange(n), chunk), int(n - valid_mask(xyz).sum())


def knn_dist2_f64(xyz, chunk=512):
    """The same statistic of the same float32 inputs in float64 (clouds without invalid points)."""
    P = np.ascontiguousarray(xyz, F32).astype(np.float64)
    n = P.shape[0]
    out = np.zeros(n)
    for s in range(0, n, chunk):
        d = P[None, :, :] - P[s:s + chunk, None, :]
        d2 = (d * d).sum(axis=2)
        d2[np.arange(d2.shape[0]), np.arange(s, s + d2.shape[0])] = np.inf
        out[s:s + chunk] = np.sort(np.partition(d2, 2, axis=1)[:, :3], axis=1).sum(axis=1) / 3.0
    return out


def fill(xyz, rgb, mean2, narrays, opacity=0.1, min_dist2=1e-7, scale_mul=1.0, scale_max=np.inf, t_center=0.0,
         t_scale=1.0):
    """The block gsr_scene_from_points builds, [narrays, n] float32, every operation float32."""
    xyz = np.ascontiguousarray(xyz, F32).reshape(-1, 3)
    n = xyz.shape[0]
    soa = np.zeros((narrays, n), F32)
    soa.view(np.uint32)[0:3] = xyz.T.view(np.uint32) if n else 0      # the bits, NaN payloads too
    soa[3] = F32(opacity)
    with np.errstate(over="ignore", invalid="ignore"):
        s = np.minimum(np.sqrt(np.maximum(np.asarray(mean2, F32), F32(min_dist2))) * F32(scale_mul), F32(scale_max))
        soa[4:7] = s.astype(F32)
        soa[7] = 1.0
        c = np.full((n, 3), 0.5, F32) if rgb is None else np.ascontiguousarray(rgb, F32).reshape(-1, 3)
        soa[11:14] = ((c - F32(0.5)) / SH_C0).T
    if narrays == 49:
        soa[38] = F32(t_center)
        soa[39] = F32(t_scale)
    return soa


# ---------------------------------------------------------------- clouds

def _dir(rng, n):
    v = rng.normal(0, 1, (n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def clustered(rng, n, clusters=40, decades=4.0):
    """Gaussian clusters in the unit cube whose radii span `decades` decades."""
    c = rng.uniform(0, 1, (clusters, 3))
    r = 10.0 ** rng.uniform(-1 - decades, -1, clusters)
    k = rng.integers(0, clusters, n)
    return (c[k] + rng.normal(0, 1, (n, 3)) * r[k][:, None]).astype(F32)


def with_outliers(rng, xyz, share, factors=(1e3,)):
    """`share` of the points moved out to `factors` times the extent, in random directions."""
    xyz = np.array(xyz, F32)
    n = xyz.shape[0]
    k = max(len(factors), int(round(n * share)))
    idx = rng.choice(n, min(k, n), replace=False)
    ext = float(np.ptp(xyz, axis=0).max()) or 1.0
    f = np.resize(np.asarray(factors, np.float64), idx.size)
    xyz[idx] = (xyz.mean(axis=0) + _dir(rng, idx.size) * (ext * f)[:, None]).astype(F32)
    return xyz


def clouds(rng, n):
    """name -> float32 [n, 3] cloud; 'nonfinite' has max(3, n // 100) points (every point below
    n = 3) with one coordinate NaN, +inf or -inf."""
    u = rng.uniform(0, 1, (n, 3)).astype(F32)
    out = {"uniform": u, "clustered": clustered(rng, n)}
    p = u.copy(); p[:, 2] = F32(0.25); out["plane"] = p
    t = rng.uniform(0, 1, n)
    out["line"] = (np.float64([0.1, 0.2, 0.3]) + t[:, None] * np.float64([1.0, 0.5, -0.25])).astype(F32)
    out["identical"] = np.tile(F32([0.3, -1.5, 2.0]), (n, 1))
    h = (n + 1) // 2
    out["duplicated"] = np.concatenate([u[:h], u[:h]])[:n][rng.permutation(n)]
    side = int(np.ceil(n ** (1 / 3)))
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)
    out["lattice"] = g[rng.permutation(g.shape[0])[:n]].astype(F32)
    two = rng.normal(0, 1, (n, 3)); two[n // 2:] += 1e6
    out["two_far_clusters"] = two.astype(F32)
    out["outliers"] = with_outliers(rng, clustered(rng, n), 0.005, (1e3, 1e9))
    out["huge"] = (rng.uniform(-1, 1, (n, 3)) * 3e19).astype(F32)
    out["offset"] = (1e4 + rng.uniform(0, 1, (n, 3))).astype(F32)
    nf = clustered(rng, n)
    k = max(3, n // 100) if n >= 3 else n
    idx = rng.choice(n, min(k, n), replace=False)
    bad = np.resize(F32([np.nan, np.inf, -np.inf]), idx.size)
    nf[idx, rng.integers(0, 3, idx.size)] = bad
    out["nonfinite"] = nf
    return out
