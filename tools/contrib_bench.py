#!/usr/bin/env python3
"""Cost of a contrib frame's blend (gsr_render_contrib) against the exact blend of
gsr_render, interleaved in ONE process on one scene, one frame at a time: after a warm-up
of sustained frames, every round renders one frame per setting, synchronises and reads
that frame's GSR_STAGE_BLEND time (HIP events around the blend launch), so clock and
thermal drift hit all settings alike.

Settings: the exact blend (render(), knob 22 = 0: the yardstick), the default fast blend
(render(), knob 22 = 1, for orientation), and render_contrib with all four outputs, the
count only, and the id plane only; then the weight only, the max only and the three
statistics without the id plane, which separate the statistics' costs.  The accumulators
are zeroed before every contrib frame (outside the timed stage).

    python tools/contrib_bench.py [--config 2] [--frames 200] [--warm-seconds 1.0]
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

KNOB_BLEND_EXP = 22


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warm-seconds", type=float, default=1.0)
    args = ap.parse_args()
    import numpy as np
    import torch
    import bench
    import gaussianrenderer_amd as gsr

    n, W, H, seed = bench.CONFIGS[args.config]
    d = os.path.join(tempfile.gettempdir(), "gsr_bench")
    os.makedirs(d, exist_ok=True)
    ply = os.path.join(d, f"config{args.config}_n{n}_s{seed}.ply")
    if not os.path.exists(ply):
        gsr.write_synthetic_ply(ply, n, seed)
    scene = gsr.Scene.from_ply(ply)
    cam = gsr.make_camera(position=(0.0, 0.0, 4.0), fov_y=50.0, aspect=W / H)
    stream = torch.cuda.current_stream().cuda_stream
    out = torch.empty(3 * W * H, dtype=torch.float32, device="cuda")
    count = torch.zeros(n, dtype=torch.int32, device="cuda")
    weight = torch.zeros(n, dtype=torch.int64, device="cuda")
    wmax = torch.zeros(n, dtype=torch.int32, device="cuda")
    ident = torch.empty(W * H, dtype=torch.int32, device="cuda")
    r = gsr.Renderer()

    def plain(mode):
        def go():
            r.set_tuning(KNOB_BLEND_EXP, mode)
            return r.render(scene, cam, W, H, out.data_ptr(), stream=stream)
        return go

    def contrib(c, w, m, i):
        def go():
            for on, buf in ((c, count), (w, weight), (m, wmax)):
                if on:
                    buf.zero_()
            return r.render_contrib(scene, cam, W, H, count_ptr=count.data_ptr() if c else None,
                                    weight_ptr=weight.data_ptr() if w else None,
                                    max_ptr=wmax.data_ptr() if m else None, id_ptr=ident.data_ptr() if i else None,
                                    stream=stream)
        return go

    settings = [("exact_blend", plain(0)), ("fast_blend", plain(1)), ("contrib_all", contrib(True, True, True, True)),
                ("contrib_count", contrib(True, False, False, False)),
                ("contrib_id", contrib(False, False, False, True)),
                # what separates the reductions from their atomics: each statistic alone, and the
                # three statistics without the id plane
                ("contrib_weight", contrib(False, True, False, False)),
                ("contrib_max", contrib(False, False, True, False)),
                ("contrib_count_weight_max", contrib(True, True, True, False))]

    # (a context's first frames can overflow the pair buffer: render until one is complete)
    def complete(go):
        go()
        while r.sync() != 0:
            go()

    # the count alone is the all-outputs count
    complete(contrib(True, True, True, True))
    ref = count.cpu().numpy().copy()
    composited = int((ref != 0).sum())
    takes = int(ref.astype(np.int64).sum())
    complete(contrib(True, False, False, False))
    identical = bool(np.array_equal(count.cpu().numpy(), ref))
    # warm-up: sustained frames of every setting
    t0 = time.time()
    while time.time() - t0 < args.warm_seconds:
        for _, go in settings:
            go()
        r.sync()
    while r.sync() != 0:
        plain(0)()
    ms = {name: [] for name, _ in settings}
    r.set_timing(1)
    r.stage_times()
    for _ in range(args.frames):
        for name, go in settings:
            go()
            r.sync()
            t, frames = r.stage_times()
            assert frames == 1, frames
            ms[name].append(t["blend"])
    r.set_timing(0)
    rep = {}
    for name, v in ms.items():
        a = np.sort(np.array(v))
        rep[name] = {"median_ms": round(float(np.median(a)), 4), "mean_ms": round(float(a.mean()), 4),
                     "p10_ms": round(float(a[len(a) // 10]), 4), "p90_ms": round(float(a[(9 * len(a)) // 10]), 4)}
    base = rep["exact_blend"]["median_ms"]
    for name in rep:
        rep[name]["ratio_to_exact"] = round(rep[name]["median_ms"] / base, 3)
    print(json.dumps({"config": args.config, "n": n, "W": W, "H": H, "frames_per_setting": args.frames,
                      "count_alone_identical_to_all_outputs": identical, "gaussians_composited": composited,
                      "takes": takes, "blend_stage": rep}, indent=1))


if __name__ == "__main__":
    main()
