#!/usr/bin/env python3
"""Cost of an aux frame's blend (gsr_render_aux) against the exact blend of gsr_render,
interleaved in ONE process on one scene, one frame at a time: after a warm-up of
sustained frames, every round renders one frame per setting, synchronises and reads that
frame's GSR_STAGE_BLEND time (HIP events around the blend launch), so clock and thermal
drift hit all settings alike.

Settings: the exact blend (render(), knob 22 = 0: the yardstick), the default fast blend
(render(), knob 22 = 1, for orientation), and render_aux with colour + alpha + depth, the
same plus 8 features, and alpha + depth only; then 1 and 4 features (both the 4-channel
kernel) and 5 (the 8-channel kernel), which separate the feature gathers from the channels'
arithmetic.

    python tools/aux_bench.py [--config 2] [--frames 200] [--warm-seconds 1.0]
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
    alpha = torch.empty(W * H, dtype=torch.float32, device="cuda")
    depth = torch.empty(W * H, dtype=torch.float32, device="cuda")
    feats = torch.rand(8 * n, dtype=torch.float32, device="cuda")
    fout = torch.empty(8 * W * H, dtype=torch.float32, device="cuda")
    r = gsr.Renderer()

    def plain(mode):
        def go():
            r.set_tuning(KNOB_BLEND_EXP, mode)
            return r.render(scene, cam, W, H, out.data_ptr(), stream=stream)
        return go

    def aux(colour, nfeat):
        def go():
            return r.render_aux(scene, cam, W, H, out_ptr=out.data_ptr() if colour else None,
                                alpha_ptr=alpha.data_ptr(), depth_ptr=depth.data_ptr(),
                                features_ptr=feats.data_ptr() if nfeat else None, nfeat=nfeat,
                                feat_out_ptr=fout.data_ptr() if nfeat else None, stream=stream)
        return go

    settings = [("exact_blend", plain(0)), ("fast_blend", plain(1)), ("aux_colour_alpha_depth", aux(True, 0)),
                ("aux_colour_alpha_depth_8feat", aux(True, 8)), ("aux_alpha_depth", aux(False, 0)),
                # the same instantiations with fewer distinct arrays (the padding channels repeat
                # the last array: same arithmetic and LDS traffic, fewer gathered lines)
                ("aux_colour_alpha_depth_1feat", aux(True, 1)), ("aux_colour_alpha_depth_4feat", aux(True, 4)),
                ("aux_colour_alpha_depth_5feat", aux(True, 5))]
    # the aux colour image is the exact blend's
    # (a context's first frames can overflow the pair buffer: render until one is complete)
    def complete(go):
        go()
        while r.sync() != 0:
            go()

    complete(plain(0))
    ref = out.cpu().numpy().copy()
    out.zero_()
    complete(aux(True, 8))
    identical = bool(np.array_equal(out.cpu().numpy().view(np.uint32), ref.view(np.uint32)))
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
                      "aux_colour_identical_to_exact": identical, "blend_stage": rep}, indent=1))


if __name__ == "__main__":
    main()
