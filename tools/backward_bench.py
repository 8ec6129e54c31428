#!/usr/bin/env python3
"""Cost of a backward frame's blend (gsr_render_backward) against the exact blend of
gsr_render and against gsr_render_contrib with all four outputs, interleaved in ONE process
on one scene, one frame at a time (tools/contrib_bench.py's method): after a warm-up of
sustained frames, every round renders one frame per setting, synchronises and reads that
frame's GSR_STAGE_BLEND time, so clock and thermal drift hit all settings alike.

Settings: the exact blend (render(), knob 22 = 0: the yardstick), render_contrib with all
four outputs, and render_backward with g = ones on the image and the alpha for (a) colour +
opacity and (b) all four outputs; then the conic + centre pair alone, which separates the
geometry's cost.  The gradient planes are zeroed before every backward frame (outside the
timed stage).  Also printed: an upper bound of the float atomics a frame issues, four blocks
per (tile, splat) pair of the frame's tile lists times the components asked for.

    python tools/backward_bench.py [--config 2] [--frames 200] [--warm-seconds 1.0]
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
COMPONENTS = {"color": 3, "opacity": 1, "conic": 4, "center": 2}


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
    g_image = torch.ones(3 * W * H, dtype=torch.float32, device="cuda")
    g_alpha = torch.ones(W * H, dtype=torch.float32, device="cuda")
    grads = {k: torch.zeros(c * n, dtype=torch.float32, device="cuda") for k, c in COMPONENTS.items()}
    r = gsr.Renderer()

    def plain():
        r.set_tuning(KNOB_BLEND_EXP, 0)
        return r.render(scene, cam, W, H, out.data_ptr(), stream=stream)

    def contrib():
        for buf in (count, weight, wmax):
            buf.zero_()
        return r.render_contrib(scene, cam, W, H, count_ptr=count.data_ptr(), weight_ptr=weight.data_ptr(),
                                max_ptr=wmax.data_ptr(), id_ptr=ident.data_ptr(), stream=stream)

    def backward(*what):
        def go():
            for k in what:
                grads[k].zero_()
            return r.render_backward(scene, cam, W, H, grad_image_ptr=g_image, grad_alpha_ptr=g_alpha,
                                     stream=stream, **{k + "_ptr": grads[k] for k in what})
        return go

    settings = [("exact_blend", plain), ("contrib_all", contrib),
                ("backward_color_opacity", backward("color", "opacity")),
                ("backward_all", backward(*COMPONENTS)),
                ("backward_conic_center", backward("conic", "center"))]

    # (a context's first frames can overflow the pair buffer: render until one is complete)
    def complete(go):
        go()
        while r.sync() != 0:
            go()

    complete(backward(*COMPONENTS))
    pairs = int(r.pair_count())
    full = {k: v.cpu().numpy().copy() for k, v in grads.items()}
    touched = int((full["opacity"] != 0).sum())
    finite = bool(all(np.isfinite(v).all() for v in full.values()))
    # colour + opacity alone against the all-outputs planes (float atomics: not bit for bit)
    complete(backward("color", "opacity"))
    dev = max(float(np.abs(grads[k].cpu().numpy() - full[k]).max() / max(np.abs(full[k]).max(), 1e-30))
              for k in ("color", "opacity"))
    t0 = time.time()
    while time.time() - t0 < args.warm_seconds:
        for _, go in settings:
            go()
        r.sync()
    while r.sync() != 0:
        plain()
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
    for name in rep:
        rep[name]["ratio_to_exact"] = round(rep[name]["median_ms"] / rep["exact_blend"]["median_ms"], 3)
        rep[name]["ratio_to_contrib_all"] = round(rep[name]["median_ms"] / rep["contrib_all"]["median_ms"], 3)
    print(json.dumps({"config": args.config, "n": n, "W": W, "H": H, "frames_per_setting": args.frames,
                      "tile_pairs": pairs, "gaussians_with_gradient": touched, "all_finite": finite,
                      "color_opacity_alone_max_rel_dev_from_all": dev,
                      "atomic_bytes_upper_bound": {"color_opacity": pairs * 4 * 4 * 4, "all": pairs * 4 * 10 * 4},
                      "blend_stage": rep}, indent=1))


if __name__ == "__main__":
    main()
