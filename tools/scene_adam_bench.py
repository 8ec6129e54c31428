#!/usr/bin/env python3
"""Cost of the fused in-place Adam step of a scene block (Scene.adam_step, include/gsr.h "scene
optimisation") against two yardsticks taken in the same run: a device-to-device copy of the
block (gsr_scene_copy: 8 B per element, so a dense step's 28 B per element are 3.5 x its bytes)
and torch.optim.Adam (fused, or foreach where this torch has no fused Adam) on ONE float32
tensor of narrays x n elements.  Interleaved in ONE process: after a warm-up of sustained work,
every round runs each setting once between two HIP events, so clock and thermal drift hit all
settings alike.  The gradient planes are restored before every timed call, outside the events.

Settings, per scene (config 2: 1M x 38 arrays; config 3: the 5M stand-in):
  scene_copy         gsr_scene_copy of the block into a buffer allocated once
  dense_all          every group active, random non-zero gradients: g, x, m, v read, x, m, v written
  skip_zero          every group active, GSR_ADAM_SKIP_ZERO, the gradients of one
                     render_backward_scene frame of the bench camera (a Gaussian no pixel
                     composited has zero gradients)
  skip_zero_clear    the same with GSR_ADAM_ZERO_GRADS
  skip_zero_runs     skip_zero on the same frame's gradients with the touched Gaussians moved to
                     the front, as in a block ordered by visibility (Scene.gather): whole waves
                     of zero gradients, which leave after loading g alone
  dense_clear        dense_all with GSR_ADAM_ZERO_GRADS (32 B per element)
  position_sh_dc     only position and sh_dc active (6 planes), dense
  torch_adam         torch.optim.Adam(fused=True) step on one narrays x n float32 tensor

    python tools/scene_adam_bench.py [--configs 2 3] [--rounds 20] [--warm-seconds 1.0]
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

PLANES = {"position": 3, "opacity": 1, "scale": 3, "rot": 4, "sh": 27}
LRS = {"lr_position": 1.6e-6, "lr_opacity": 5e-4, "lr_scale": 5e-5, "lr_rot": 1e-5, "lr_sh_dc": 2.5e-5,
       "lr_sh_rest": 1.25e-6}   # small: hundreds of timed steps must leave a sane scene


def run_config(config, rounds, warm_seconds):
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
    copy_buf = torch.empty(block_bytes, dtype=torch.uint8, device="cuda")

    def planes(fill):
        return {k: fill(p * n) for k, p in PLANES.items()}

    gen = torch.Generator(device="cuda").manual_seed(11)
    zeros = lambda size: torch.zeros(size, dtype=torch.float32, device="cuda")
    g = planes(zeros)
    m, v = planes(zeros), planes(zeros)
    g_random = planes(lambda size: torch.randn(size, device="cuda", generator=gen) * 1e-3)

    # one real backward frame of the bench camera: zero for every Gaussian no pixel composited
    cam = gsr.make_camera(position=(0.0, 0.0, 4.0), fov_y=50.0, aspect=W / H)
    r = gsr.Renderer()
    grad_image = torch.randn(3 * W * H, device="cuda", generator=gen)
    g_frame = planes(zeros)
    while True:
        for t in g_frame.values():
            t.zero_()
        r.render_backward_scene(scene, cam, W, H, grad_image_ptr=grad_image, stream=stream,
                                **{k + "_ptr": t for k, t in g_frame.items()})
        if r.sync() == 0:
            break
    r.close()
    touched = int((g_frame["opacity"] != 0).sum().item())
    nonzero = sum(int((t != 0).sum().item()) for t in g_frame.values()) / (na * n)
    order = torch.argsort((g_frame["opacity"] == 0).to(torch.uint8), stable=True)
    g_runs = {k: t.view(PLANES[k], n)[:, order].contiguous().view(-1) for k, t in g_frame.items()}

    step = [0]

    def adam(source, lrs, **flags):
        def restore():
            for k in g:
                g[k].copy_(source[k])

        def go():
            step[0] += 1
            scene.adam_step(g, m, v, step=step[0], stream=stream, **lrs, **flags)
        return restore, go

    def scene_copy():
        gsr.check(L.gsr_scene_copy(copy_buf.data_ptr(), scene.ptr, na, n, stream), "gsr_scene_copy")

    # torch's own Adam on one tensor of the block's size
    param = torch.randn(na * n, device="cuda", generator=gen).requires_grad_(True)
    param.grad = torch.randn(na * n, device="cuda", generator=gen) * 1e-3
    try:
        opt, torch_kind = torch.optim.Adam([param], lr=1e-5, eps=1e-15, fused=True), "fused"
        opt.step()
    except Exception:
        opt, torch_kind = torch.optim.Adam([param], lr=1e-5, eps=1e-15, foreach=True), "foreach"
        opt.step()

    nothing = lambda: None
    two = {"lr_position": LRS["lr_position"], "lr_sh_dc": LRS["lr_sh_dc"]}
    settings = [("scene_copy", nothing, scene_copy, 8 * na * n),
                ("dense_all",) + adam(g_random, LRS) + (28 * na * n,),
                ("skip_zero",) + adam(g_frame, LRS, skip_zero=True) + (None,),
                ("skip_zero_clear",) + adam(g_frame, LRS, skip_zero=True, zero_grads=True) + (None,),
                ("skip_zero_runs",) + adam(g_runs, LRS, skip_zero=True) + (None,),
                ("dense_clear",) + adam(g_random, LRS, zero_grads=True) + (32 * na * n,),
                ("position_sh_dc",) + adam(g_random, two) + (28 * 6 * n,),
                ("torch_adam", nothing, opt.step, 28 * na * n)]

    settings[1][1]()
    t0 = time.time()
    while time.time() - t0 < warm_seconds:   # warm-up: sustained copies and dense steps
        scene_copy()
        settings[1][2]()
        torch.cuda.synchronize()
    ms = {s[0]: [] for s in settings}
    for _ in range(rounds):
        for name, restore, go, _ in settings:
            restore()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            go()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))

    soa = scene.download()
    sane = bool(np.isfinite(soa).all())
    rep = {}
    for name, _, _, moved in settings:
        a = np.array(ms[name])
        e = {"median_ms": round(float(np.median(a)), 4), "min_ms": round(float(a.min()), 4),
             "p90_ms": round(float(np.sort(a)[(9 * len(a)) // 10]), 4)}
        if moved:
            e["moved_GBps"] = round(moved / (e["median_ms"] * 1e-3) / 1e9, 1)
        rep[name] = e
    base = rep["scene_copy"]["median_ms"]
    for e in rep.values():
        e["ratio_to_scene_copy"] = round(e["median_ms"] / base, 3)
        e["ratio_to_torch"] = round(e["median_ms"] / rep["torch_adam"]["median_ms"], 3)
    scene.free()
    return {"config": config, "n": n, "narrays": na, "block_MB": round(block_bytes / 1e6, 1), "rounds": rounds,
            "torch_adam": torch_kind, "frame_touched_gaussians": touched, "frame_nonzero_fraction": round(nonzero, 4),
            "scene_finite_after": sane,
            "dense_over_3p5_copies": round(rep["dense_all"]["median_ms"] / (3.5 * base), 3), "settings": rep}


def table(res):
    lines = [f"config {res['config']}: n = {res['n']:,} x {res['narrays']} arrays, block {res['block_MB']} MB, "
             f"{res['rounds']} interleaved rounds; the backward frame touched {res['frame_touched_gaussians']:,} "
             f"Gaussians ({100 * res['frame_nonzero_fraction']:.1f} % of the gradient elements non-zero); "
             f"torch Adam: {res['torch_adam']}; scene finite afterwards: {res['scene_finite_after']}",
             f"{'setting':<18}{'median ms':>11}{'min ms':>9}{'p90 ms':>9}{'GB/s moved':>12}{'x copy':>8}{'x torch':>9}"]
    for name, e in res["settings"].items():
        lines.append(f"{name:<18}{e['median_ms']:>11}{e['min_ms']:>9}{e['p90_ms']:>9}{e.get('moved_GBps', ''):>12}"
                     f"{e['ratio_to_scene_copy']:>8}{e['ratio_to_torch']:>9}")
    lines.append(f"dense_all / (3.5 x scene_copy) = {res['dense_over_3p5_copies']}")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, nargs="+", default=[2, 3])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warm-seconds", type=float, default=1.0)
    ap.add_argument("--label", default="", help="what to name in the report: the commit and the box")
    ap.add_argument("--out", default=None, help="also write the tables to this file")
    args = ap.parse_args()
    import torch
    results = [run_config(c, args.rounds, args.warm_seconds) for c in args.configs]
    head = f"tools/scene_adam_bench.py  {args.label}  device: {torch.cuda.get_device_name(0)}"
    text = "\n\n".join([head] + [table(r) for r in results]) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(json.dumps({"label": args.label, "results": results}))


if __name__ == "__main__":
    main()
