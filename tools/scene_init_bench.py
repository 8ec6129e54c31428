#!/usr/bin/env python3
"""Cost of scene initialisation from a point cloud (points_knn_dist2, Scene.from_points;
include/gsr.h "scene initialisation") against a device copy of the bytes each call must touch and
against the only thing a user could do before without a host round trip, a chunked brute force
in torch.  Interleaved in ONE process as tools/scene_densify_bench.py does: after a warm-up of
sustained work, every round runs each setting once between two HIP events, so clock and thermal
drift hit all settings alike; rounds continue until every setting has a second of device time or
--rounds is reached.

Per size (1M and 5M points, the sizes of configs 2 and 3) and cloud:
  uniform            a uniform cube
  clustered          Gaussian clusters whose densities span four decades
  outliers           the clustered cloud with 0.1 % of the points at 1,000 x the extent
Settings:
  knn                points_knn_dist2 (interleaved [n, 3] input), against
  copy_16n           a device copy of the 12 n bytes in + 4 n out it must touch
  from_points        Scene.from_points with colours (38 arrays; synchronous, allocates), against
  copy_block         a device copy of those 16 n bytes plus the block's 38 x 4 n
  torch_brute        (1M, uniform only, run once) cdist over row chunks + topk on the device
Checks at the timed sizes: 1,024 sampled rows of the output equal the numpy twin's rows
(tests/_points_ref.py knn_rows) bit for bit; the block's scale plane equals the twin's fill of
the device's statistic.

    python tools/scene_init_bench.py [--sizes 1000000 5000000] [--rounds 40] [--warm-seconds 1.0]
                                     [--label TEXT] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def make_cloud(name, n, seed):
    import numpy as np
    import _points_ref as ref
    rng = np.random.default_rng(seed)
    if name == "uniform":
        return rng.uniform(0, 1, (n, 3)).astype(np.float32)
    xyz = ref.clustered(rng, n, clusters=400)
    if name == "outliers":
        xyz = ref.with_outliers(rng, xyz, 0.001, (1e3,))
    return xyz


def torch_brute(torch, d_xyz, chunk=4096):
    """mean of the three smallest squared distances, self excluded: cdist over row chunks + topk.
    Not the rule's arithmetic (cdist rounds differently): a cost yardstick only."""
    n = d_xyz.shape[0]
    out = torch.empty(n, dtype=torch.float32, device="cuda")
    for s in range(0, n, chunk):
        d = torch.cdist(d_xyz[s:s + chunk], d_xyz)
        out[s:s + chunk] = (d.topk(4, dim=1, largest=False).values[:, 1:] ** 2).mean(dim=1)
    return out


def run_cloud(name, n, rounds, warm_seconds, brute):
    import numpy as np
    import torch
    import _points_ref as ref
    import gaussianrenderer_amd as gsr

    xyz = make_cloud(name, n, n % 1000 + len(name))
    rgb = np.random.default_rng(7).uniform(0, 1, (n, 3)).astype(np.float32)
    d_xyz, d_rgb = torch.from_numpy(xyz).cuda(), torch.from_numpy(rgb).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    nbytes = gsr.points_knn_scratch_bytes(n)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    out = torch.zeros(n, dtype=torch.float32, device="cuda")
    block_bytes = int(gsr.lib().gsr_scene_bytes(38, n))
    c16 = [torch.empty(4 * n, dtype=torch.float32, device="cuda") for _ in range(2)]
    cblk = [torch.empty(16 * n + block_bytes, dtype=torch.uint8, device="cuda") for _ in range(2)]

    def device_copy(pair):
        def go():
            pair[1].copy_(pair[0])
        return go

    settings = [
        ("knn", lambda: gsr.points_knn_dist2(d_xyz, n, out, scratch, nbytes, stream=stream)),
        ("copy_16n", device_copy(c16)),
        ("from_points", lambda: gsr.Scene.from_points(d_xyz, n, d_rgb, stream=stream)),
        ("copy_block", device_copy(cblk)),
    ]

    # faster and different is not faster: sampled rows against the twin, the block against the fill
    settings[0][1]()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    rows = np.random.default_rng(11).choice(n, 1024, replace=False)
    with ThreadPoolExecutor(8) as pool:     # numpy releases the GIL: the O(n) rows in parallel
        want = np.concatenate(list(pool.map(lambda r: ref.knn_rows(xyz, r, chunk=8), np.array_split(rows, 32))))
    rows_equal = bool(np.array_equal(got[rows].view(np.uint32), want.view(np.uint32)))
    sc = gsr.Scene.from_points(d_xyz, n, d_rgb, stream=stream)
    soa = sc.download()
    sc.free()
    fill_equal = bool(np.array_equal(soa.view(np.uint32), ref.fill(xyz, rgb, got, 38).view(np.uint32)))
    del soa

    t0 = time.time()
    while time.time() - t0 < warm_seconds:
        settings[0][1]()
        settings[1][1]()
        torch.cuda.synchronize()
    ms = {k: [] for k, _ in settings}
    for _ in range(rounds):
        for k, go in settings:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            res = go()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
            if isinstance(res, gsr.Scene):
                res.free()      # outside the timed span
        if len(ms["knn"]) >= 5 and min(sum(v) for v in ms.values()) >= 1000.0:
            break

    rep = {}
    for k, _ in settings:
        a = np.array(ms[k])
        rep[k] = {"median_ms": round(float(np.median(a)), 4), "min_ms": round(float(a.min()), 4),
                  "p90_ms": round(float(np.sort(a)[(9 * len(a)) // 10]), 4), "rounds": len(a)}
    for k, against in (("knn", "copy_16n"), ("from_points", "copy_block")):
        rep[k]["against"] = against
        rep[k]["ratio"] = round(rep[k]["median_ms"] / rep[against]["median_ms"], 2)
    if brute:
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b = torch_brute(torch, d_xyz)
        e1.record()
        e1.synchronize()
        t = e0.elapsed_time(e1)
        rel = float(((b - out).abs() / out.clamp_min(1e-30)).median().item())
        rep["torch_brute"] = {"median_ms": round(t, 1), "rounds": 1, "against": "knn",
                              "ratio": round(t / rep["knn"]["median_ms"], 1), "median_rel_diff_to_knn": rel}
    return {"cloud": name, "n": n, "scratch_MB": round(nbytes / 1e6, 1), "block_MB": round(block_bytes / 1e6, 1),
            "sample_rows_equal_twin": rows_equal, "block_equals_fill_twin": fill_equal, "settings": rep}


def table(res):
    lines = [f"{res['cloud']}: n = {res['n']:,}, scratch {res['scratch_MB']} MB, block {res['block_MB']} MB; "
             f"1,024 sampled rows == twin: {res['sample_rows_equal_twin']}; block == fill twin: "
             f"{res['block_equals_fill_twin']}",
             f"{'setting':<14}{'median ms':>11}{'min ms':>10}{'p90 ms':>10}{'rounds':>8}   against"]
    for k, e in res["settings"].items():
        vs = f"   {e['ratio']} x {e['against']}" if "against" in e else ""
        lines.append(f"{k:<14}{e['median_ms']:>11}{e.get('min_ms', ''):>10}{e.get('p90_ms', ''):>10}{e['rounds']:>8}{vs}")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1_000_000, 5_000_000])
    ap.add_argument("--clouds", nargs="+", default=["uniform", "clustered", "outliers"])
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--warm-seconds", type=float, default=1.0)
    ap.add_argument("--brute-max", type=int, default=1_000_000, help="largest size the torch brute force runs at")
    ap.add_argument("--label", default="", help="what to name in the report: the commit and the box")
    ap.add_argument("--out", default=None, help="also write the tables to this file")
    args = ap.parse_args()
    import torch
    results = []
    for n in args.sizes:
        for name in args.clouds:
            results.append(run_cloud(name, n, args.rounds, args.warm_seconds, name == "uniform" and n <= args.brute_max))
        by = {r["cloud"]: r["settings"]["knn"]["median_ms"] for r in results if r["n"] == n}
        if "outliers" in by and "clustered" in by:
            results[-1]["outliers_over_clustered"] = round(by["outliers"] / by["clustered"], 2)
    head = f"tools/scene_init_bench.py  {args.label}  device: {torch.cuda.get_device_name(0)}"
    parts = [head]
    for r in results:
        parts.append(table(r))
        if "outliers_over_clustered" in r:
            parts.append(f"n = {r['n']:,}: knn on the outlier cloud / on the clean clustered cloud = "
                         f"{r['outliers_over_clustered']}")
    text = "\n\n".join(parts) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(json.dumps({"label": args.label, "results": results}))


if __name__ == "__main__":
    main()
