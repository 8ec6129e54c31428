#!/usr/bin/env python3
"""The shared preprocess kernel alone against the per-frame one, for a kernel trace or a
counter pass (rocprofv3 ... -- python3 tools/pre_shared_probe.py [--config 2] [--reps 20]):
four distinct orbit cameras; `reps` x 4 plain gsr_render calls (k_preprocess, one camera,
nothing else on the device when it starts), then `reps` four-frame gsr_render_path calls on
four lanes, each drained before the next (k_preprocess_multi<.,4> is the call's first kernel).

    python3 tools/pre_shared_probe.py --summarize <dir with the rocprofv3 csv files>

prints, per preprocess kernel, the launches and the mean / median duration of the kernel
trace, and the mean of every counter of a counter pass (per launch and per Gaussian).
"""
from __future__ import annotations

import argparse
import collections
import csv
import glob
import os
import re
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kname(name):
    m = re.search(r"k_preprocess\w*<[^>]*>", name)
    return m.group(0) if m else None


def summarize(root, n):
    dur = collections.defaultdict(list)
    for f in glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if kname(r["Kernel_Name"]):
                dur[kname(r["Kernel_Name"])].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for k, v in sorted(dur.items()):
        print(f"{k:32s} launches {len(v):4d}  mean {statistics.mean(v):8.2f} us  median {statistics.median(v):8.2f} us")
    pmc = collections.defaultdict(lambda: collections.defaultdict(list))
    for f in glob.glob(os.path.join(root, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if kname(r["Kernel_Name"]):
                pmc[kname(r["Kernel_Name"])][r["Counter_Name"]].append(float(r["Counter_Value"]))
    for k, d in sorted(pmc.items()):
        for c, v in sorted(d.items()):
            print(f"{k:32s} {c:16s} launches {len(v):4d}  mean {statistics.mean(v):.6g}  per Gaussian {statistics.mean(v) / n:.5g}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--summarize")
    a = ap.parse_args()
    import bench
    n, W, H, seed = bench.CONFIGS[a.config]
    if a.summarize:
        return summarize(a.summarize, n)
    import torch
    import gaussianrenderer_amd as gsr
    from gaussianrenderer_amd import multi
    d = os.path.join(tempfile.gettempdir(), "gsr_bench")
    os.makedirs(d, exist_ok=True)
    ply = os.path.join(d, f"config{a.config}_n{n}_s{seed}.ply")
    if not os.path.exists(ply):
        gsr.write_synthetic_ply(ply + ".tmp", n, seed)
        os.replace(ply + ".tmp", ply)
    scene = gsr.Scene.from_ply(ply)
    cams = [multi.orbit_camera(i, W, H) for i in range(4)]
    outs = [torch.empty(3 * W * H, dtype=torch.float32, device="cuda") for _ in cams]
    ptrs = [o.data_ptr() for o in outs]
    r = gsr.Renderer()
    r.set_frames_in_flight(4)
    for _ in range(3):                      # workspaces at their high-water marks, splitters seeded
        r.render_path(scene, cams, W, H, ptrs)
        r.sync()
    for _ in range(a.reps):
        for cam, p in zip(cams, ptrs):
            r.render(scene, cam, W, H, p)
            r.sync()
    for _ in range(a.reps):
        r.render_path(scene, cams, W, H, ptrs)
        r.sync()
    print("shared launches", r.get_tuning(gsr.TUNE_PATH_SHARED_LAUNCHES))


if __name__ == "__main__":
    main()
