#!/usr/bin/env python3
"""Cost of device-side scene editing (Scene.select / Scene.gather, include/gsr.h "scene
editing") against a device-to-device copy of the same block (gsr_scene_copy: the yardstick of
the keep-all case) and against the host round trip callers had before (download, numpy index,
upload), interleaved in ONE process: after a warm-up of sustained work, every round runs each
setting once between two HIP events, so clock and thermal drift hit all settings alike.

Settings, per scene (config 2: 1M x 38 arrays; config 3: the 5M stand-in):
  scene_copy        gsr_scene_copy of the block into a buffer allocated once
  select_all        Scene.select, keep-all mask: the pure move cost (compaction, allocation,
                    gather; the call is synchronous, the events span all of it)
  select_half       Scene.select, random 50 % mask
  select_contrib    Scene.select, mask count > 0 of one render_contrib frame: the pruning case
  gather_perm       Scene.gather, random permutation: one cache line per element and plane,
                    inherent to the SoA layout
  compact_*         mask_indices alone, on the three masks (three launches, a readback)
  kernel_*          gather_planes of the 38 planes into a buffer allocated once, with the index
                    lists above: the gather kernel alone, without compaction and allocation
  host_round_trip   download + numpy fancy index by the contrib mask + upload (wall clock)

    python tools/scene_ops_bench.py [--configs 2 3] [--rounds 20] [--warm-seconds 1.0]
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

    # the pruning mask: one contrib frame of the bench camera
    cam = gsr.make_camera(position=(0.0, 0.0, 4.0), fov_y=50.0, aspect=W / H)
    r = gsr.Renderer()
    count = torch.zeros(n, dtype=torch.int32, device="cuda")
    while True:
        count.zero_()
        r.render_contrib(scene, cam, W, H, count_ptr=count.data_ptr(), stream=stream)
        if r.sync() == 0:
            break
    gen = torch.Generator(device="cuda").manual_seed(7)
    masks = {"all": torch.ones(n, dtype=torch.uint8, device="cuda"),
             "half": (torch.rand(n, device="cuda", generator=gen) < 0.5).to(torch.uint8),
             "contrib": (count != 0).to(torch.uint8)}
    kept = {k: int(v.sum().item()) for k, v in masks.items()}
    lists = {k: torch.nonzero(v).flatten().to(torch.int32) for k, v in masks.items()}
    lists["perm"] = torch.randperm(n, device="cuda", generator=gen).to(torch.int32)
    kept["perm"] = n
    r.close()

    copy_buf = torch.empty(block_bytes, dtype=torch.uint8, device="cuda")
    stride = (n + 63) // 64 * 64
    planes_buf = torch.empty(na * stride, dtype=torch.float32, device="cuda")
    idx_buf = torch.empty(n, dtype=torch.int32, device="cuda")
    arrays_ptr = scene.ptr + 256

    def scene_copy():
        gsr.check(L.gsr_scene_copy(copy_buf.data_ptr(), scene.ptr, na, n, stream), "gsr_scene_copy")

    def select(mask):
        def go():
            return scene.select(masks[mask], idx_buf, stream=stream)
        return go

    def gather_perm():
        return scene.gather(lists["perm"], n, stream=stream)

    def compact(mask):
        def go():
            gsr.mask_indices(masks[mask], n, idx_buf, stream=stream)
        return go

    def kernel(which):
        def go():
            m = kept[which]
            gsr.gather_planes(planes_buf, (m + 63) // 64 * 64, arrays_ptr, stride, na, 4, n, lists[which], m,
                              stream=stream)
        return go

    settings = ([("scene_copy", scene_copy, "all")] +
                [(f"select_{k}", select(k), k) for k in ("all", "half", "contrib")] +
                [("gather_perm", gather_perm, "perm")] +
                [(f"compact_{k}", compact(k), None) for k in ("all", "half", "contrib")] +
                [(f"kernel_{k}", kernel(k), k) for k in ("all", "half", "contrib", "perm")])

    # the device results are what numpy gives
    soa = scene.download()
    s = scene.select(masks["contrib"], idx_buf, stream=stream)
    keep_host = masks["contrib"].cpu().numpy().astype(bool)
    identical = bool(np.array_equal(s.download().view(np.uint32), soa[:, keep_host].view(np.uint32)) and
                     np.array_equal(idx_buf[:s.n].cpu().numpy(), np.flatnonzero(keep_host)))
    s.free()

    # warm-up: sustained copies and gathers
    t0 = time.time()
    while time.time() - t0 < warm_seconds:
        scene_copy()
        kernel("all")()
        torch.cuda.synchronize()
    ms = {name: [] for name, _, _ in settings}
    wall = {name: [] for name, _, _ in settings}
    for _ in range(rounds):
        for name, go, _ in settings:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            w0 = time.perf_counter()
            e0.record()
            res = go()
            e1.record()
            e1.synchronize()
            wall[name].append((time.perf_counter() - w0) * 1e3)
            ms[name].append(e0.elapsed_time(e1))
            if res is not None:
                res.free()      # outside the timed span (hipFree waits for the device)

    host = []
    for _ in range(host_reps):
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        full = scene.download()
        t1 = time.perf_counter()
        cut = np.ascontiguousarray(full[:, keep_host])
        t2 = time.perf_counter()
        up = gsr.Scene.from_soa(cut)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        host.append(((t3 - w0) * 1e3, (t1 - w0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))
        up.free()

    rep = {}
    base = None
    for name, _, which in settings:
        a = np.array(ms[name])
        e = {"median_ms": round(float(np.median(a)), 4), "min_ms": round(float(a.min()), 4),
             "p90_ms": round(float(np.sort(a)[(9 * len(a)) // 10]), 4),
             "wall_median_ms": round(float(np.median(wall[name])), 4)}
        if which is not None:   # bytes the move reads and writes: 2 x m x narrays x 4
            moved = 2 * kept[which] * na * 4
            e["kept"] = kept[which]
            e["moved_GBps"] = round(moved / (e["median_ms"] * 1e-3) / 1e9, 1)
        rep[name] = e
        if name == "scene_copy":
            base = e["median_ms"]
    for name in rep:
        rep[name]["ratio_to_scene_copy"] = round(rep[name]["median_ms"] / base, 3)
    h = np.array(host)
    rep["host_round_trip"] = {"median_ms": round(float(np.median(h[:, 0])), 1),
                              "download_ms": round(float(np.median(h[:, 1])), 1),
                              "numpy_index_ms": round(float(np.median(h[:, 2])), 1),
                              "upload_ms": round(float(np.median(h[:, 3])), 1), "kept": kept["contrib"],
                              "ratio_to_scene_copy": round(float(np.median(h[:, 0])) / base, 1),
                              "ratio_to_select_contrib": round(float(np.median(h[:, 0])) /
                                                               rep["select_contrib"]["median_ms"], 1)}
    scene.free()
    return {"config": config, "n": n, "narrays": na, "block_MB": round(block_bytes / 1e6, 1), "rounds": rounds,
            "select_identical_to_numpy": identical, "settings": rep}


def table(res):
    lines = [f"config {res['config']}: n = {res['n']:,} x {res['narrays']} arrays, block {res['block_MB']} MB, "
             f"{res['rounds']} interleaved rounds, select == numpy: {res['select_identical_to_numpy']}",
             f"{'setting':<18}{'kept':>10}{'median ms':>11}{'min ms':>9}{'p90 ms':>9}{'wall ms':>9}"
             f"{'GB/s moved':>12}{'x copy':>8}"]
    for name, e in res["settings"].items():
        lines.append(f"{name:<18}{e.get('kept', ''):>10}{e['median_ms']:>11}{e.get('min_ms', ''):>9}"
                     f"{e.get('p90_ms', ''):>9}{e.get('wall_median_ms', ''):>9}{e.get('moved_GBps', ''):>12}"
                     f"{e['ratio_to_scene_copy']:>8}")
    h = res["settings"]["host_round_trip"]
    lines.append(f"host_round_trip = download {h['download_ms']} + numpy index {h['numpy_index_ms']} + upload "
                 f"{h['upload_ms']} ms; {h['ratio_to_select_contrib']} x select_contrib")
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
    head = f"tools/scene_ops_bench.py  {args.label}  device: {torch.cuda.get_device_name(0)}"
    text = "\n\n".join([head] + [table(r) for r in results]) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(json.dumps({"label": args.label, "results": results}))


if __name__ == "__main__":
    main()
