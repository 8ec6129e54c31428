"""spans_check.py (analysis only, not product, not test): a numpy restatement of
tile_row_spans (gsr_kernels.hip) on the oracle's preprocess records.  For each scene it
prints the fraction of (tile, splat) rect pairs the spans keep and the largest alpha any
DROPPED pair reaches on an in-box pixel of its tile (must stay < 1e-3: the drop is then
invisible).  `python tools/sim/spans_check.py c1` (config 1, four cameras), `c2` (config
2) or `wide` (the scenes of tests/_wide_scenes.py that tests/test_gpu_wide.py runs the spans
on: large, tilted and clipped splats, centres far off screen)."""
import os, sys, tempfile, numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import gaussianrenderer_amd as gsr, _oracle as orc
from test_gpu_parity import max_alpha_on_tiles, CAMS, cam_for
f32 = np.float32
def spans_np(want, W, H):
    v = want["status"] == 2
    n = len(want)
    cx = want["px_x"].astype(f32); cy = want["px_y"].astype(f32)
    a, b, c, e = [want["inv_covar"][:, i].astype(f32) for i in range(4)]
    op = want["opacity"].astype(f32)
    with np.errstate(all="ignore"):
        h = f32(0.5) * (b + c)
        pd = (a > 0) & (e > 0) & ((a * e - h * h) > f32(1e-4) * (a * e))
        cut = (np.log2(op * f32(1000)) * f32(1.38629436111989061)) * f32(1.00001) + f32(1e-3)
        S = np.abs(a) + np.abs(b) + np.abs(c) + np.abs(e)
        ok = pd & np.isfinite(cut) & np.isfinite(S) & v
        det = a * e - h * h
        ax0, ay0, ax1, ay1 = [want["aabb"][:, i].astype(np.int64) for i in range(4)]
        M = np.maximum(np.maximum(np.abs(ax0.astype(f32) - cx), np.abs(ax1.astype(f32) - cx)), np.maximum(np.abs(ay0.astype(f32) - cy), np.abs(ay1.astype(f32) - cy)))
        C = cut + (f32(4e-6) * S * M * M + f32(1e-3))
        rdet = f32(1) / det; ra = f32(1) / a
        xr = np.sqrt(C * e * rdet); ym = np.sqrt(C * a * rdet); yr = -h * xr * (f32(1) / e)
        k = a * e * rdet
        rel = np.sqrt(f32(6e-7) * (k + f32(1))) + f32(1e-4)
        padx = f32(1 / 64) + rel * xr; ymp = ym * (f32(1) + rel) + f32(1 / 64)
        aC = a * C
    tx, ty = (W + 15) // 16, (H + 15) // 16
    tx0 = ax0 // 16; tx1 = np.minimum(tx - 1, ax2 := ax1 // 16); ty0 = ay0 // 16; ty1 = np.minimum(ty - 1, ay1 // 16)
    w = tx1 - tx0 + 1
    code = np.zeros(n, np.uint32)
    for r in range(4):
        tyr = ty0 + r
        act = ok & (tyr <= ty1)
        y0 = np.maximum(tyr * 16, ay0); y1 = np.minimum(tyr * 16 + 15, ay1)
        with np.errstate(all="ignore"):
            dy0 = y0.astype(f32) - cy; dy1 = y1.astype(f32) - cy
            inr = ~((dy0 > ymp) | (dy1 < -ymp))
            u0 = np.minimum(np.maximum(dy0, -ym), ym); u1 = np.minimum(np.maximum(dy1, -ym), ym)
            inR = (yr >= u0) & (yr <= u1)
            uR = np.where(yr < u0, u0, u1)
            R = np.where(inR, xr, (-h * uR + np.sqrt(np.maximum(aC - det * uR * uR, f32(0)))) * ra)
            inL = (-yr >= u0) & (-yr <= u1)
            uL = np.where(-yr < u0, u0, u1)
            L = np.where(inL, -xr, (-h * uL - np.sqrt(np.maximum(aC - det * uL * uL, f32(0)))) * ra)
            xl = np.maximum(cx + L - padx, ax0.astype(f32)); xh = np.minimum(cx + R + padx, ax1.astype(f32))
            good = inr & (xl <= xh)
            c0 = np.where(good, np.maximum(tx0, np.floor(xl * f32(1 / 16)).astype(np.int64)), tx1 + 1)
            c1 = np.where(good, np.minimum(tx1, np.floor(xh * f32(1 / 16)).astype(np.int64)), tx0 - 1)
        empty = c0 > c1
        sl = np.where(empty, np.minimum(w, 3), np.minimum(c0 - tx0, 3)); sr = np.where(empty, np.minimum(w, 3), np.minimum(tx1 - c1, 3))
        code |= np.where(act, (sl | (sr << 2)).astype(np.uint32) << np.uint32(4 * r), 0).astype(np.uint32)
    return code, tx0, tx1, ty0
def listed(full, code, tx0, tx1, ty0, W):
    tx = (W + 15) // 16
    tile = (full >> np.uint64(32)).astype(np.int64); idx = (full & np.uint64(0xFFFFFFFF)).astype(np.int64)
    col = tile % tx; row = tile // tx
    ro = row - ty0[idx]
    sp = np.where(ro < 4, (code[idx] >> (4 * np.minimum(ro, 3)).astype(np.uint32)) & 0xf, 0)
    c0 = tx0[idx] + (sp & 3); c1 = tx1[idx] - (sp >> 2)
    return (col >= c0) & (col <= c1)
def synthetic(n, seed):
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "s.ply"); gsr.write_synthetic_ply(p, n, seed)
        return gsr.read_ply(p)
def report(label, soa, cam, W, H, k=3.0):
    from _wide_scenes import rect_pairs as fast_pairs
    want = orc.preprocess(soa, cam, W, H, k)
    full = fast_pairs(want, orc.expected_depth_order(want), W, H)
    code, tx0, tx1, ty0 = spans_np(want, W, H)
    keep = listed(full, code, tx0, tx1, ty0, W)
    dropped = full[~keep]
    al = max_alpha_on_tiles(want, dropped, W)
    print(f"{label}: pairs {full.size} kept {keep.mean():.3f} dropped {dropped.size} ({1 - keep.mean():.3f}) max alpha of dropped {al.max() if al.size else 0:.3e}", flush=True)
cfg = sys.argv[1] if len(sys.argv) > 1 else "c1"
if cfg == "c1":
    W, H = 640, 480; soa = synthetic(10_000, 1)
    for ci, kw in enumerate(CAMS):
        report(f"config 1 camera {ci}", soa, cam_for(gsr, W, H, **kw), W, H)
elif cfg == "c2":
    W, H = 1920, 1080
    report("config 2", synthetic(1_000_000, 2), gsr.make_camera(position=(0, 0, 4), fov_y=50, aspect=W / H), W, H)
elif cfg == "wide":
    import _wide_scenes as ws
    W, H = ws.W, ws.H
    for name in ("slabs", "needles", "stack", "huge"):
        for ci, kw in enumerate(CAMS):
            report(f"{name} camera {ci} k 3", ws.scene(name), cam_for(gsr, W, H, **kw), W, H)
    for k in (8.0, 1.0):
        for ci in (0, 2):
            report(f"slabs camera {ci} k {k:g}", ws.scene("slabs"), cam_for(gsr, W, H, **CAMS[ci]), W, H, k)
    for seed in ws.GRAZE_SEEDS:
        report(f"graze seed {seed}", ws.graze(seed), cam_for(gsr, W, H), W, H)
else:
    sys.exit("usage: spans_check.py c1 | c2 | wide")
