"""numpy twin of the scene densification (include/gsr.h "scene densification"): the statistic,
the classification, the expansion order, the split children's arithmetic, the masked moment
gather and the opacity reset.  In float32 every numpy operation below is one rounding, in the
operation order the header states, so the device results are compared bit for bit; with
dtype=np.float64 the same code is the real-valued map that test_densify_ref.py pins to a
restatement of 3DGS.  The normals come from the library's host export (gsr_densify_normals),
which is the host build of the code the split kernel runs."""
import numpy as np

A_X, A_OPACITY, A_SCALE0, A_ROT0 = 0, 3, 4, 7
CHUNK = 1024   # kDensifyChunk: sources per workgroup of the expansion's kernels

CFG_3DGS = dict(grad_threshold=0.0002, scale_split=0.05, min_opacity=0.005, prune_scale_max=float("inf"),
                split_shrink=1.6, seed=0)


# ---------------------------------------------------------------- Philox4x32-10 and Box-Muller

def philox4x32_10(counter, key):
    """The Random123 generator on uint32 arrays: counter (4, N), key (2,) or (2, N) -> (4, N)."""
    c = [np.asarray(x, np.uint64) for x in counter]
    k = [np.asarray(x, np.uint64) for x in key]
    M0, M1, W0, W1, MASK = (np.uint64(v) for v in (0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF))
    S = np.uint64(32)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> S) ^ c[1] ^ k[0], p1 & MASK, (p0 >> S) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + W0) & MASK, (k[1] + W1) & MASK]
    return np.stack([np.broadcast_to(x, c[1].shape) for x in c]).astype(np.uint32)


def child_words(seed, index, child):
    """x0..x3 of the children (index[j], child[j]) under seed: (4, N) uint32."""
    index, child = np.broadcast_arrays(np.asarray(index, np.uint32), np.asarray(child, np.uint32))
    zero = np.zeros(index.shape, np.uint32)
    return philox4x32_10([index, child, zero, zero], [np.uint32(seed & 0xFFFFFFFF), np.uint32(seed >> 32)])


def box_muller64(x):
    """The header's Box-Muller in float64 on the exact u, v and 2 pi: (N, 3)."""
    u = lambda w: ((w >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    v = lambda w: (w >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    r1, a1 = np.sqrt(-2.0 * np.log(u(x[0]))), 2.0 * np.pi * v(x[1])
    r2, a2 = np.sqrt(-2.0 * np.log(u(x[2]))), 2.0 * np.pi * v(x[3])
    return np.stack([r1 * np.cos(a1), r1 * np.sin(a1), r2 * np.cos(a2)], axis=1)


# ---------------------------------------------------------------- the statistic

def accumulate(center, W, H, accum, seen):
    """(accum', seen', bad) after one gsr_densify_accumulate of the (2, n) centre planes."""
    gx, gy = np.asarray(center, np.float32)
    finite = np.isfinite(gx) & np.isfinite(gy)
    touch = finite & ~((gx == 0) & (gy == 0))
    with np.errstate(all="ignore"):
        a = gx * (np.float32(0.5) * np.float32(W))
        b = gy * (np.float32(0.5) * np.float32(H))
        norm = np.sqrt((a * a) + (b * b))
        accum2 = np.where(touch, np.asarray(accum, np.float32) + norm, accum).astype(np.float32)
    seen2 = np.where(touch, np.asarray(seen, np.uint32) + np.uint32(1), seen).astype(np.uint32)
    return accum2, seen2, int((~finite).sum())


# ---------------------------------------------------------------- the densify call

def classify(soa, accum, seen, cfg, dtype=np.float32):
    """Per source: (outputs 0 / 1 / 2, split?) by the header's comparisons in `dtype`."""
    f = dtype
    soa = np.asarray(soa, f)
    accum, seen = np.asarray(accum, f), np.asarray(seen, np.uint32)
    with np.errstate(all="ignore"):
        avg = np.where(seen != 0, accum / np.where(seen != 0, seen, 1).astype(f), f(0))
        hot = avg >= f(cfg["grad_threshold"])
        smax = np.fmax(np.fmax(soa[A_SCALE0], soa[A_SCALE0 + 1]), soa[A_SCALE0 + 2])
        split = hot & (smax > f(cfg["scale_split"]))
        sout = np.where(split, smax / f(cfg["split_shrink"]), smax)
        pruned = (soa[A_OPACITY] < f(cfg["min_opacity"])) | (sout > f(cfg["prune_scale_max"]))
    outs = np.where(pruned, 0, np.where(hot, 2, 1))
    return outs, split, hot, pruned


def rotation(q, f):
    """Row-major rotation matrix entries (9, N) of the normalised quaternions q (4, N): the
    preprocess's expressions (math.cu:153-164) in their operation order."""
    qw, qx, qy, qz = (np.asarray(x, f) for x in q)
    one, two = f(1), f(2)
    with np.errstate(all="ignore"):
        qn = np.sqrt(qx * qx + qy * qy + qz * qz + qw * qw)
        qx, qy, qz, qw = qx / qn, qy / qn, qz / qn, qw / qn
        return [one - two * qy * qy - two * qz * qz, two * qx * qy - two * qw * qz, two * qx * qz + two * qw * qy,
                two * qx * qy + two * qw * qz, one - two * qx * qx - two * qz * qz, two * qy * qz - two * qw * qx,
                two * qx * qz - two * qw * qy, two * qy * qz + two * qw * qx, one - two * qx * qx - two * qy * qy]


def children(soa, idx, z, shrink, dtype=np.float32):
    """The block columns of one child of each parent idx[j] with normals z (len, 3)."""
    f = dtype
    par = np.asarray(soa, f)[:, idx].copy()
    z = np.asarray(z, f)
    s = par[A_SCALE0:A_SCALE0 + 3].copy()
    R = rotation(par[A_ROT0:A_ROT0 + 4], f)
    with np.errstate(all="ignore"):
        t = [z[:, c] * s[c] for c in range(3)]
        for r in range(3):
            par[A_X + r] = par[A_X + r] + ((R[3 * r] * t[0] + R[3 * r + 1] * t[1]) + R[3 * r + 2] * t[2])
            par[A_SCALE0 + r] = s[r] / f(shrink)
    return par


def densify(soa, accum, seen, cfg, normals, dtype=np.float32):
    """gsr_scene_densify: (block (narrays, n_out), src int32, kind uint8, report dict).
    normals(index, child) -> (len, 3) array: the sampler (gsr.densify_normals under the seed)."""
    soa = np.asarray(soa, dtype)
    n = soa.shape[1]
    outs, split, hot, pruned = classify(soa, accum, seen, cfg, dtype)
    src = np.repeat(np.arange(n, dtype=np.int32), outs)
    second = np.zeros(src.size, bool)
    second[1:] = src[1:] == src[:-1]                      # the second output of its source
    kind = (np.where(split[src], 2, 0) + second).astype(np.uint8)
    block = soa[:, src].copy()
    for k in (0, 1):
        at = np.flatnonzero(kind == 2 + k)
        if at.size:
            block[:, at] = children(soa, src[at], normals(src[at], np.full(at.size, k)), cfg["split_shrink"], dtype)
    report = dict(n_out=int(src.size), kept=int((~pruned & ~hot).sum()), cloned=int((~pruned & hot & ~split).sum()),
                  split=int((~pruned & split).sum()), pruned=int(pruned.sum()))
    return block, src, kind, report


# ---------------------------------------------------------------- companions

def gather_planes(src_planes, idx, kind):
    """gsr_densify_gather_planes: (planes, bad) with the clamp of the indices that are read."""
    src_planes = np.asarray(src_planes, np.float32)
    n = src_planes.shape[1]
    idx, kind = np.asarray(idx, np.int64), np.asarray(kind, np.uint8)
    read = kind == 0
    bad = int((read & ((idx < 0) | (idx >= n))).sum())
    out = src_planes[:, np.clip(idx, 0, n - 1)].copy()
    out[:, ~read] = 0.0
    return out, bad


def reset_opacity(soa, cap):
    out = np.asarray(soa, np.float32).copy()
    out[A_OPACITY] = np.fmin(out[A_OPACITY], np.float32(cap))
    return out
