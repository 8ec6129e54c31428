#!/usr/bin/env python3
"""Cost of gsr_render_backward_aux's depth and feature channels against gsr_render_backward with
all four outputs, of gsr_project_backward_aux against gsr_project_backward, and of the fused
gsr_render_backward_scene_aux against the two-call chain: interleaved in ONE process on one
scene, one frame at a time (tools/backward_bench.py's method), so clock and thermal drift hit
all settings alike.

Blend settings (GSR_STAGE_BLEND time of the frame, which for the aux call holds the -Z and
feature-pack kernels too), g = ones on every plane given, all outputs of the setting asked for:
  backward_all     gsr_render_backward, colour + opacity + conic + centre (the yardstick)
  aux_none         gsr_render_backward_aux with no aux input or output (the same kernel)
  aux_depth        + d_grad_depth and d_z
  aux_feat4        + 4 features: d_grad_feat and d_feat
  aux_depth_feat8  + depth and 8 features
  aux_depth_feat8_only  the same inputs, d_z and d_feat the only outputs: one sweep, no gathers
The gradient planes are zeroed before every frame, outside the timed stage.

Projection and fused settings (device time between two events on the stream):
  project / project_aux            ten planes / ten planes and d_z
  chain / fused                    memset of 11 planes + render_backward_aux + project_backward_aux
                                   / render_backward_scene_aux with a caller's scratch

The whole measurement runs --repeats times; the report gives every repeat's ratio beside the
median over all frames, which is the run-to-run spread inside one process.

    python tools/backward_aux_bench.py [--config 2] [--frames 100] [--repeats 3] [--warm-seconds 1.0]
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

COMPONENTS = {"color": 3, "opacity": 1, "conic": 4, "center": 2}
SCENE_GROUPS = {"position": 3, "opacity": 1, "scale": 3, "rot": 4, "sh": 27}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2)
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
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
    ts = torch.cuda.current_stream()
    stream = ts.cuda_stream
    f32 = dict(dtype=torch.float32, device="cuda")
    g_image, g_alpha, g_depth = torch.ones(3 * W * H, **f32), torch.ones(W * H, **f32), torch.ones(W * H, **f32)
    g_feat = torch.ones(8 * W * H, **f32)
    feats = torch.from_numpy(np.random.default_rng(1).standard_normal((8, n)).astype(np.float32)).cuda()
    grads = {k: torch.zeros(c * n, **f32) for k, c in COMPONENTS.items()}
    grads["z"], grads["feat_grad"] = torch.zeros(n, **f32), torch.zeros(8 * n, **f32)
    planes = torch.zeros(11 * n, **f32)          # the record planes of the projection and fused settings
    outs = {k: torch.zeros(c * n, **f32) for k, c in SCENE_GROUPS.items()}
    out_kw = {k + "_ptr": v for k, v in outs.items()}
    r = gsr.Renderer()

    def zero(names):
        for k in names:
            grads[k].zero_()

    def backward_all():
        zero(COMPONENTS)
        return r.render_backward(scene, cam, W, H, grad_image_ptr=g_image, grad_alpha_ptr=g_alpha, stream=stream,
                                 **{k + "_ptr": grads[k] for k in COMPONENTS})

    def aux(depth, nfeat, record=True):
        names = (list(COMPONENTS) if record else []) + (["z"] if depth else []) + (["feat_grad"] if nfeat else [])

        def go():
            zero(names)
            kw = {k + "_ptr": grads[k] for k in names}
            if depth:
                kw["grad_depth_ptr"] = g_depth
            if nfeat:
                kw.update(grad_feat_ptr=g_feat, features_ptr=feats, nfeat=nfeat)
            return r.render_backward_aux(scene, cam, W, H, grad_image_ptr=g_image, grad_alpha_ptr=g_alpha,
                                         stream=stream, **kw)
        return go

    blend = [("backward_all", backward_all), ("aux_none", aux(False, 0)), ("aux_depth", aux(True, 0)),
             ("aux_feat4", aux(False, 4)), ("aux_depth_feat8", aux(True, 8)),
             ("aux_depth_feat8_only", aux(True, 8, record=False))]

    def complete(go):     # (a context's first frames can overflow the pair buffer)
        go()
        while r.sync() != 0:
            go()

    # the record planes the projection settings read: one complete frame with depth
    complete(aux(True, 8))
    dz_touched = int((grads["z"] != 0).sum())
    finite = bool(all(torch.isfinite(v).all() for v in grads.values()))
    src = torch.cat([grads[k] for k in COMPONENTS] + [grads["z"]]).clone()
    rec = {k: src[o * n:(o + c) * n] for k, o, c in (("d_color", 0, 3), ("d_opacity", 3, 1), ("d_conic", 4, 4),
                                                     ("d_center", 8, 2), ("d_z", 10, 1))}
    rec_kw = {k + "_ptr": v for k, v in rec.items()}
    ten_kw = {k: v for k, v in rec_kw.items() if k != "d_z_ptr"}
    aux_in = dict(grad_image_ptr=g_image, grad_alpha_ptr=g_alpha, grad_depth_ptr=g_depth)

    def project():
        return r.project_backward(scene, cam, W, H, stream=stream, **ten_kw, **out_kw)

    def project_aux():
        return r.project_backward_aux(scene, cam, W, H, stream=stream, **rec_kw, **out_kw)

    def chain():
        planes.zero_()
        p = {k + "_ptr": planes[o * n:(o + c) * n] for k, o, c in (("color", 0, 3), ("opacity", 3, 1), ("conic", 4, 4),
                                                                  ("center", 8, 2), ("z", 10, 1))}
        r.render_backward_aux(scene, cam, W, H, stream=stream, **aux_in, **p)
        q = {"d_" + k: v for k, v in p.items()}
        return r.project_backward_aux(scene, cam, W, H, stream=stream, **q, **out_kw)

    def fused():
        return r.render_backward_scene_aux(scene, cam, W, H, stream=stream, scratch_ptr=planes, **aux_in, **out_kw)

    timed = [("project", project), ("project_aux", project_aux), ("chain", chain), ("fused", fused)]

    def event_ms(go):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(ts)
        go()
        b.record(ts)
        r.sync()
        b.synchronize()
        return a.elapsed_time(b)

    t0 = time.time()
    while time.time() - t0 < args.warm_seconds:
        for _, go in blend + timed:
            go()
        r.sync()
    while r.sync() != 0:
        backward_all()
    ms = {name: [[] for _ in range(args.repeats)] for name, _ in blend + timed}
    for rep in range(args.repeats):
        r.set_timing(1)
        r.stage_times()
        for _ in range(args.frames):
            for name, go in blend:
                go()
                r.sync()
                t, frames = r.stage_times()
                assert frames == 1, frames
                ms[name][rep].append(t["blend"])
        r.set_timing(0)
        for _ in range(args.frames):
            for name, go in timed:
                ms[name][rep].append(event_ms(go))
    med = lambda v: float(np.median(np.array(v)))  # noqa: E731
    report = {}
    for name, base in [(nm, "backward_all") for nm, _ in blend] + [("project", "project"), ("project_aux", "project"),
                                                                  ("chain", "chain"), ("fused", "chain")]:
        every = [x for v in ms[name] for x in v]
        report[name] = {"median_ms": round(med(every), 4),
                        "p10_ms": round(float(np.percentile(every, 10)), 4),
                        "p90_ms": round(float(np.percentile(every, 90)), 4),
                        "ratio_to": base,
                        "ratio": round(med(every) / med([x for v in ms[base] for x in v]), 3),
                        "ratio_per_repeat": [round(med(ms[name][k]) / med(ms[base][k]), 3)
                                             for k in range(args.repeats)]}
    print(json.dumps({"config": args.config, "n": n, "W": W, "H": H, "frames_per_setting_and_repeat": args.frames,
                      "repeats": args.repeats, "tile_pairs": int(r.pair_count()),
                      "gaussians_with_depth_gradient": dz_touched, "all_finite": finite, "timings": report}, indent=1))


if __name__ == "__main__":
    main()
