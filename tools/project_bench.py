#!/usr/bin/env python3
"""Cost of the projection's backward pass (gsr_project_backward, k_project_backward) beside its
two natural yardsticks, the same frame's preprocess (GSR_STAGE_PREPROCESS) and the backward
blend (gsr_render_backward's GSR_STAGE_BLEND), and of the fused gsr_render_backward_scene
against gsr_render_backward alone; everything interleaved in ONE process on one scene
(tools/backward_bench.py's method), so clock and thermal drift hit all settings alike.

The projection kernel is timed with every output requested, for three upstreams: a real
frame's record gradients (g = ones on the image and the alpha), an all-zero upstream (every
Gaussian leaves before its scene arrays are loaded) and an all-non-zero upstream (every
Gaussian with a record does the full work).  Each sample is the device time between two events
around --calls back-to-back calls, divided by their number.  The whole-call times (fused,
render_backward alone with its planes zeroed outside the window) are event times of one call.
Also printed: the bytes the kernel has to move, 40 + 12 narrays per Gaussian that is not
skipped (ten upstream floats, narrays scene floats, a read-modify-write of as many planes).

    python tools/project_bench.py [--config 2] [--frames 100] [--calls 10] [--warm-seconds 1.0]
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

NARRAYS = 38
GROUPS = {"position": (0, 3), "opacity": (3, 4), "scale": (4, 7), "rot": (7, 11), "sh": (11, 38)}
RECORD = {"color": (0, 3), "opacity": (3, 4), "conic": (4, 8), "center": (8, 10)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--calls", type=int, default=10)
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
    g_image = torch.ones(3 * W * H, dtype=torch.float32, device="cuda")
    g_alpha = torch.ones(W * H, dtype=torch.float32, device="cuda")
    planes = torch.zeros((10, n), dtype=torch.float32, device="cuda")      # the record gradients
    grads = torch.zeros((NARRAYS, n), dtype=torch.float32, device="cuda")  # the scene gradients
    rec_ptrs = {k + "_ptr": planes[a:b] for k, (a, b) in RECORD.items()}
    out_ptrs = {k + "_ptr": grads[a:b] for k, (a, b) in GROUPS.items()}
    r = gsr.Renderer()

    def backward():
        return r.render_backward(scene, cam, W, H, grad_image_ptr=g_image, grad_alpha_ptr=g_alpha, stream=stream,
                                 **rec_ptrs)

    def fused():
        return r.render_backward_scene(scene, cam, W, H, grad_image_ptr=g_image, grad_alpha_ptr=g_alpha,
                                       scratch_ptr=planes, stream=stream, **out_ptrs)

    # (a context's first frames can overflow the pair buffer: render until one is complete)
    planes.zero_()
    backward()
    while r.sync() != 0:
        planes.zero_()
        backward()
    upstream = {"real": planes.clone(), "zero": torch.zeros_like(planes), "nonzero": torch.ones_like(planes)}
    live = int((upstream["real"] != 0).any(0).sum())

    def project(up):
        r.project_backward(scene, cam, W, H, stream=stream, **{"d_" + k + "_ptr": up[a:b] for k, (a, b) in RECORD.items()},
                           **out_ptrs)

    # what the three upstreams make the kernel do: Gaussians whose planes change
    moved = {}
    for name, up in upstream.items():
        grads.zero_()
        project(up)
        torch.cuda.synchronize()
        moved[name] = int((grads != 0).any(0).sum())
    finite = bool(torch.isfinite(grads).all())

    def timed(go, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            go()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / calls

    t0 = time.time()
    while time.time() - t0 < args.warm_seconds:
        r.render(scene, cam, W, H, out.data_ptr(), stream=stream)
        fused()
        for up in upstream.values():
            project(up)
        r.sync()
    while r.sync() != 0:
        fused()

    ms = {k: [] for k in ("preprocess_stage", "backward_blend_stage", "project_real", "project_zero",
                          "project_nonzero", "render_backward_call", "fused_call")}
    for _ in range(args.frames):
        r.set_timing(2)      # an event at every stage boundary
        r.stage_times()
        planes.zero_()
        backward()
        r.sync()
        t, frames = r.stage_times()
        assert frames == 1, frames
        r.set_timing(0)
        ms["preprocess_stage"].append(t["preprocess"])
        ms["backward_blend_stage"].append(t["blend"])
        for name, up in upstream.items():
            grads.zero_()
            torch.cuda.synchronize()
            ms["project_" + name].append(timed(lambda: project(up), args.calls))
        planes.zero_()
        torch.cuda.synchronize()
        ms["render_backward_call"].append(timed(backward, 1))
        r.sync()
        grads.zero_()
        torch.cuda.synchronize()
        ms["fused_call"].append(timed(fused, 1))
        r.sync()
    rep = {}
    for name, v in ms.items():
        a = np.sort(np.array(v))
        rep[name] = {"median_ms": round(float(np.median(a)), 4), "mean_ms": round(float(a.mean()), 4),
                     "p10_ms": round(float(a[len(a) // 10]), 4), "p90_ms": round(float(a[(9 * len(a)) // 10]), 4)}
    med = lambda k: rep[k]["median_ms"]  # noqa: E731
    for name in ("project_real", "project_zero", "project_nonzero"):
        rep[name]["ratio_to_preprocess"] = round(med(name) / med("preprocess_stage"), 3)
        rep[name]["ratio_to_backward_blend"] = round(med(name) / med("backward_blend_stage"), 4)
        gb = moved[name.split("_")[1]] * (40 + 12 * NARRAYS) / 1e9
        rep[name]["gbytes_needed"] = round(gb + (n - moved[name.split("_")[1]]) * 40 / 1e9, 4)
        rep[name]["gbytes_per_s"] = round(rep[name]["gbytes_needed"] / (med(name) * 1e-3), 1)
    rep["fused_call"]["ratio_to_render_backward_call"] = round(med("fused_call") / med("render_backward_call"), 4)
    print(json.dumps({"config": args.config, "n": n, "W": W, "H": H, "frames": args.frames,
                      "calls_per_project_sample": args.calls, "gaussians_with_record_gradient": live,
                      "gaussians_moved": moved, "all_finite": finite, "times": rep}, indent=1))


if __name__ == "__main__":
    main()
