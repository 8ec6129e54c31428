#!/usr/bin/env python3
"""Cost of device-side densification (Scene.densify, densify_accumulate, Scene.reset_opacity;
include/gsr.h "scene densification") against the calls it is built from and the host round trip
it replaces, interleaved in ONE process as tools/scene_ops_bench.py does: after a warm-up of
sustained work, every round runs each setting once between two HIP events, so clock and thermal
drift hit all settings alike.

Settings, per scene (config 2: 1M x 38 arrays; config 3: the 5M stand-in):
  scene_copy        gsr_scene_copy of the block into a buffer allocated once (a device memcpy)
  select_all        Scene.select with a keep-all mask: the same output block as densify_kept
                    (compaction, allocation, gather; synchronous; code the densification leaves
                    as it was)
  densify_kept      Scene.densify with grad_threshold = +inf and the prunes off: every source
                    kept, so the difference to select_all is the classification and the expansion
  densify_mix       Scene.densify on a statistic and thresholds that clone ~5 %, split ~5 % and
                    prune ~5 % of the sources (the report's counts are printed)
  accumulate        densify_accumulate with every Gaussian composited (the dense case), against
  copy_16n          a device copy of the 16 n bytes it touches (2 centre planes, accum, seen)
  reset_opacity     Scene.reset_opacity with both moment planes, against
  copy_12n          a device copy of the 12 n bytes it touches (opacity, m, v)
  host_round_trip   what densify_mix replaces: download, the same classification, expansion and
                    children in numpy (normals from numpy's generator), upload (wall clock)

    python tools/scene_densify_bench.py [--configs 2 3] [--rounds 20] [--warm-seconds 1.0]
                                        [--label TEXT] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

INF = float("inf")


def numpy_densify(soa, accum, seen, cfg, rng):
    """The host's densify in float32 numpy: classification, stable expansion, children."""
    import numpy as np
    n = soa.shape[1]
    avg = np.where(seen != 0, accum / np.maximum(seen, 1).astype(np.float32), np.float32(0))
    hot = avg >= np.float32(cfg["grad_threshold"])
    smax = soa[4:7].max(axis=0)
    split = hot & (smax > np.float32(cfg["scale_split"]))
    sout = np.where(split, smax / np.float32(cfg["split_shrink"]), smax)
    pruned = (soa[3] < np.float32(cfg["min_opacity"])) | (sout > np.float32(cfg["prune_scale_max"]))
    outs = np.where(pruned, 0, np.where(hot, 2, 1))
    src = np.repeat(np.arange(n, dtype=np.int32), outs)
    block = soa[:, src]
    kid = np.flatnonzero(split[src])
    par = block[:, kid]
    q = par[7:11] / np.sqrt((par[7:11] ** 2).sum(axis=0))
    w, x, y, z = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], np.float32)
    t = rng.standard_normal((3, kid.size), dtype=np.float32) * par[4:7]
    block[0:3, kid] = par[0:3] + np.einsum("rck,ck->rk", R, t)
    block[4:7, kid] = par[4:7] / np.float32(cfg["split_shrink"])
    return block


def run_config(config, rounds, warm_seconds, host_reps):
    import numpy as np
    import torch
    import bench
    import gaussianrenderer_amd as gsr

    n, W, H, seed = bench.CONFIGS[config]
    d = os.path.join(tempfile.gettempdir(), "gsr_bench")
    os.makedirs(d, exist_ok=True)
    ply = os.path.join(d, f"config{config}_n{n}_s{seed}.ply")
    if not os.path.exists(ply):
        gsr.write_synthetic_ply(ply, n, seed)
    scene = gsr.Scene.from_ply(ply)
    na = scene.narrays
    L = gsr.lib()
    stream = torch.cuda.current_stream().cuda_stream
    block_bytes = int(L.gsr_scene_bytes(na, n))
    soa = scene.download()

    # the statistic: 10 % of the sources hot; thresholds that split half of those and prune 5 %
    rng = np.random.default_rng(seed)
    hot = rng.random(n) < 0.10
    accum_h = np.where(hot, 1.0, 1e-6).astype(np.float32)
    seen_h = rng.integers(1, 4, n).astype(np.uint32)
    accum_h *= seen_h
    smax = soa[4:7].max(axis=0)
    mix = dict(grad_threshold=0.5, scale_split=float(np.median(smax[hot])), min_opacity=float(np.quantile(soa[3], 0.05)),
               prune_scale_max=INF, split_shrink=1.6, seed=seed)
    kept_cfg = dict(mix, grad_threshold=INF, min_opacity=0.0)
    accum = torch.from_numpy(accum_h).cuda()
    seen = torch.from_numpy(seen_h.view(np.int32)).cuda()
    keep_all = torch.ones(n, dtype=torch.uint8, device="cuda")
    idx_buf = torch.empty(n, dtype=torch.int32, device="cuda")
    src_buf = torch.empty(2 * n, dtype=torch.int32, device="cuda")
    kind_buf = torch.empty(2 * n, dtype=torch.uint8, device="cuda")
    copy_buf = torch.empty(block_bytes, dtype=torch.uint8, device="cuda")
    center = torch.randn(2 * n, dtype=torch.float32, device="cuda")
    acc_buf = torch.zeros(n, dtype=torch.float32, device="cuda")
    seen_buf = torch.zeros(n, dtype=torch.int32, device="cuda")
    mom = [torch.ones(n, dtype=torch.float32, device="cuda") for _ in range(2)]
    c16 = [torch.empty(4 * n, dtype=torch.float32, device="cuda") for _ in range(2)]
    c12 = [torch.empty(3 * n, dtype=torch.float32, device="cuda") for _ in range(2)]
    work = gsr.Scene.from_soa(soa)   # the reset's own block

    reports = {}

    def device_copy(pair):
        def go():
            pair[1].copy_(pair[0])
        return go

    def densify(name, cfg):
        def go():
            out, rep = scene.densify(accum, seen, src_ptr=src_buf, kind_ptr=kind_buf, stream=stream, **cfg)
            reports[name] = rep
            return out
        return go

    def scene_copy():
        gsr.check(L.gsr_scene_copy(copy_buf.data_ptr(), scene.ptr, na, n, stream), "gsr_scene_copy")

    settings = [
        ("scene_copy", scene_copy),
        ("select_all", lambda: scene.select(keep_all, idx_buf, stream=stream)),
        ("densify_kept", densify("densify_kept", kept_cfg)),
        ("densify_mix", densify("densify_mix", mix)),
        ("accumulate", lambda: gsr.densify_accumulate(center, n, W, H, acc_buf, seen_buf, stream=stream)),
        ("copy_16n", device_copy(c16)),
        ("reset_opacity", lambda: work.reset_opacity(0.01, mom[0], mom[1], stream=stream)),
        ("copy_12n", device_copy(c12)),
    ]

    # the all-kept densify is the source block
    same = scene.densify(accum, seen, **kept_cfg)[0]
    identical = bool(np.array_equal(same.download().view(np.uint32), soa.view(np.uint32)))
    same.free()

    t0 = time.time()
    while time.time() - t0 < warm_seconds:
        scene_copy()
        settings[4][1]()
        torch.cuda.synchronize()
    ms = {name: [] for name, _ in settings}
    wall = {name: [] for name, _ in settings}
    for _ in range(rounds):
        for name, go in settings:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            w0 = time.perf_counter()
            e0.record()
            res = go()
            e1.record()
            e1.synchronize()
            wall[name].append((time.perf_counter() - w0) * 1e3)
            ms[name].append(e0.elapsed_time(e1))
            if isinstance(res, gsr.Scene):
                res.free()      # outside the timed span (hipFree waits for the device)

    host = []
    hrng = np.random.default_rng(1)
    for _ in range(host_reps):
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        full = scene.download()
        a_h, s_h = accum.cpu().numpy(), seen.cpu().numpy().view(np.uint32)
        t1 = time.perf_counter()
        grown = numpy_densify(full, a_h, s_h, mix, hrng)
        t2 = time.perf_counter()
        up = gsr.Scene.from_soa(grown)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        host.append(((t3 - w0) * 1e3, (t1 - w0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, up.n))
        up.free()

    rep = {}
    for name, _ in settings:
        a = np.array(ms[name])
        rep[name] = {"median_ms": round(float(np.median(a)), 4), "min_ms": round(float(a.min()), 4),
                     "p90_ms": round(float(np.sort(a)[(9 * len(a)) // 10]), 4),
                     "wall_median_ms": round(float(np.median(wall[name])), 4)}
    base = rep["scene_copy"]["median_ms"]
    for name in rep:
        rep[name]["ratio_to_scene_copy"] = round(rep[name]["median_ms"] / base, 3)
    for name, against in (("densify_kept", "select_all"), ("accumulate", "copy_16n"), ("reset_opacity", "copy_12n")):
        rep[name]["against"] = against
        rep[name]["ratio"] = round(rep[name]["median_ms"] / rep[against]["median_ms"], 3)
    h = np.array(host, np.float64)
    assert int(h[0, 4]) == reports["densify_mix"]["n_out"], "the host's expansion has another size"
    rep["host_round_trip"] = {"median_ms": round(float(np.median(h[:, 0])), 1),
                              "download_ms": round(float(np.median(h[:, 1])), 1),
                              "numpy_ms": round(float(np.median(h[:, 2])), 1),
                              "upload_ms": round(float(np.median(h[:, 3])), 1),
                              "ratio_to_scene_copy": round(float(np.median(h[:, 0])) / base, 1),
                              "against": "densify_mix",
                              "ratio": round(float(np.median(h[:, 0])) / rep["densify_mix"]["median_ms"], 1)}
    scene.free()
    work.free()
    return {"config": config, "n": n, "narrays": na, "block_MB": round(block_bytes / 1e6, 1), "rounds": rounds,
            "kept_identical_to_source": identical, "reports": reports, "settings": rep}


def table(res):
    lines = [f"config {res['config']}: n = {res['n']:,} x {res['narrays']} arrays, block {res['block_MB']} MB, "
             f"{res['rounds']} interleaved rounds, all-kept densify == source block: {res['kept_identical_to_source']}",
             f"{'setting':<18}{'median ms':>11}{'min ms':>9}{'p90 ms':>9}{'wall ms':>9}{'x copy':>9}   against"]
    for name, e in res["settings"].items():
        vs = f"   {e['ratio']} x {e['against']}" if "against" in e else ""
        lines.append(f"{name:<18}{e['median_ms']:>11}{e.get('min_ms', ''):>9}{e.get('p90_ms', ''):>9}"
                     f"{e.get('wall_median_ms', ''):>9}{e['ratio_to_scene_copy']:>9}{vs}")
    h = res["settings"]["host_round_trip"]
    lines.append(f"host_round_trip = download {h['download_ms']} + numpy {h['numpy_ms']} + upload {h['upload_ms']} ms")
    for name, r in res["reports"].items():
        lines.append(f"{name} report: {r}")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, nargs="+", default=[2, 3])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warm-seconds", type=float, default=1.0)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--label", default="", help="what to name in the report: the commit and the box")
    ap.add_argument("--out", default=None, help="also write the tables to this file")
    args = ap.parse_args()
    import torch
    results = [run_config(c, args.rounds, args.warm_seconds, args.host_reps) for c in args.configs]
    head = f"tools/scene_densify_bench.py  {args.label}  device: {torch.cuda.get_device_name(0)}"
    text = "\n\n".join([head] + [table(r) for r in results]) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(json.dumps({"label": args.label, "results": results}))


if __name__ == "__main__":
    main()
