#!/usr/bin/env python3
"""Cost of the fused image loss (gaussianrenderer_amd.image_loss, include/gsr.h "image loss")
against yardsticks taken in the same run.  Interleaved in ONE process: after a warm-up of
sustained work, every round runs each setting once between two HIP events (starting at another
setting each round), so clock and thermal drift hit all settings alike.

Settings, per frame size (x = a random image, y = x + N(0, 0.05), weights 0.8 / 0 / 0.2):
  loss_and_grad   the four loss values and the gradient (three launches)
  value_only      the loss values alone (forward without the partial maps, and the sum)
  grad_only       the gradient alone (forward and backward launches)
  copy_3_images   three device-to-device copies of an image-sized buffer (3 * W * H floats
                  each): 12 B read and 12 B written per image element
  sub_x_y         torch.sub(x, y, out=g): one pass that reads x and y and writes a gradient-
                  sized buffer, the traffic floor of any loss gradient (12 B per element)
  torch_loss      the same loss and its backward with torch float32 ops on the same buffers
                  (3DGS's ssim(): five conv2d(padding=5, groups=3), then autograd); if this
                  torch cannot run the grouped convolution, the window as shifted slices

    python tools/image_loss_bench.py [--sizes 1920x1080 1600x1063] [--rounds 24]
                                     [--warm-seconds 1.0] [--label TEXT] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WEIGHTS = (0.8, 0.0, 0.2)
C1, C2 = 1e-4, 9e-4


def torch_loss_fn(torch, W, H, kind):
    """loss(x, y) on planar (3, H, W) tensors with torch ops; kind: 'conv2d' or 'slices'."""
    k = torch.arange(11, dtype=torch.float64)
    g = torch.exp(-(k - 5) ** 2 / (2 * 1.5 ** 2))
    g = (g / g.sum()).float().cuda()
    w2 = (g[:, None] * g[None, :]).expand(3, 1, 11, 11).contiguous()
    F = torch.nn.functional

    if kind == "conv2d":
        def win(t):
            return F.conv2d(t[None], w2, padding=5, groups=3)[0]
    else:
        def win(t):
            p = F.pad(t, (5, 5, 5, 5))
            h = sum(g[i] * p[:, :, i:i + W] for i in range(11))
            return sum(g[i] * h[:, i:i + H, :] for i in range(11))

    def loss(x, y):
        mu1, mu2 = win(x), win(y)
        s1, s2, s12 = win(x * x) - mu1 * mu1, win(y * y) - mu2 * mu2, win(x * y) - mu1 * mu2
        ssim = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))
        d = x - y
        return WEIGHTS[0] * d.abs().mean() + WEIGHTS[1] * (d * d).mean() + WEIGHTS[2] * (1 - ssim.mean())
    return loss


def run_size(W, H, rounds, warm_seconds):
    import numpy as np
    import torch
    import gaussianrenderer_amd as gsr

    n = 3 * W * H
    gen = torch.Generator(device="cuda").manual_seed(5)
    x = torch.rand(n, device="cuda", generator=gen)
    y = (x + 0.05 * torch.randn(n, device="cuda", generator=gen)).contiguous()
    grad = torch.zeros(n, device="cuda")
    loss = torch.zeros(gsr.LOSS_NVALUES, device="cuda")
    nbytes = gsr.image_loss_scratch_bytes(W, H)
    scratch = torch.empty(nbytes // 4, dtype=torch.float32, device="cuda")
    bufs = [torch.empty(n, device="cuda") for _ in range(3)]
    stream = torch.cuda.current_stream().cuda_stream
    w = dict(w_l1=WEIGHTS[0], w_l2=WEIGHTS[1], w_dssim=WEIGHTS[2])

    def loss_and_grad():
        gsr.image_loss(x, y, W, H, grad_ptr=grad, loss_ptr=loss, scratch_ptr=scratch, stream=stream, **w)

    def value_only():
        gsr.image_loss(x, y, W, H, loss_ptr=loss, scratch_ptr=scratch, stream=stream, **w)

    def grad_only():
        gsr.image_loss(x, y, W, H, grad_ptr=grad, scratch_ptr=scratch, stream=stream, **w)

    def copy_3_images():
        bufs[0].copy_(x)
        bufs[1].copy_(y)
        bufs[2].copy_(grad)

    def sub_x_y():
        torch.sub(x, y, out=bufs[0])

    xg = x.view(3, H, W).clone().requires_grad_(True)
    yv = y.view(3, H, W)
    torch_kind, fn = None, None
    for kind in ("conv2d", "slices"):
        try:
            fn = torch_loss_fn(torch, W, H, kind)
            fn(xg, yv).backward()
            torch.cuda.synchronize()
            torch_kind = kind
            break
        except Exception as e:   # this torch build has no grouped convolution for the device
            print(f"torch_loss as {kind} failed: {type(e).__name__}: {e}", file=sys.stderr)
    if torch_kind is None:
        raise RuntimeError("no torch form of the loss ran")

    def torch_loss():
        xg.grad = None
        fn(xg, yv).backward()

    # the two agree (the device call against torch's float32, loosely: this is a timing tool)
    loss_and_grad()
    torch_loss()
    torch.cuda.synchronize()
    gdiff = float((grad.view(3, H, W) - xg.grad).abs().max() / xg.grad.abs().max())
    ldiff = abs(float(loss[0]) - float(fn(xg, yv).detach()))

    settings = [("loss_and_grad", loss_and_grad, None), ("value_only", value_only, None), ("grad_only", grad_only, None),
                ("copy_3_images", copy_3_images, 24 * n), ("sub_x_y", sub_x_y, 12 * n), ("torch_loss", torch_loss, None)]
    t0 = time.time()
    while time.time() - t0 < warm_seconds:   # warm-up: sustained copies and loss calls
        copy_3_images()
        loss_and_grad()
        torch.cuda.synchronize()
    ms = {s[0]: [] for s in settings}
    for rnd in range(rounds):
        # a round starts at another setting each time: whatever the first call after an idle
        # gap pays is spread over all of them
        for name, go, _ in settings[rnd % len(settings):] + settings[:rnd % len(settings)]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            go()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))

    rep = {}
    for name, _, moved in settings:
        a = np.array(ms[name])
        e = {"median_ms": round(float(np.median(a)), 4), "min_ms": round(float(a.min()), 4),
             "p90_ms": round(float(np.sort(a)[(9 * len(a)) // 10]), 4)}
        if moved:
            e["moved_GBps"] = round(moved / (e["median_ms"] * 1e-3) / 1e9, 1)
        rep[name] = e
    for e in rep.values():
        e["ratio_to_copy3"] = round(e["median_ms"] / rep["copy_3_images"]["median_ms"], 3)
        e["ratio_to_sub"] = round(e["median_ms"] / rep["sub_x_y"]["median_ms"], 3)
        e["ratio_to_torch"] = round(e["median_ms"] / rep["torch_loss"]["median_ms"], 4)
    return {"W": W, "H": H, "image_MB": round(4 * n / 1e6, 1), "scratch_MB": round(nbytes / 1e6, 1), "rounds": rounds,
            "torch_loss": torch_kind, "grad_rel_diff_to_torch": gdiff, "loss_diff_to_torch": ldiff, "settings": rep}


def table(res):
    lines = [f"{res['W']} x {res['H']}: image {res['image_MB']} MB (3 planes), scratch {res['scratch_MB']} MB, "
             f"{res['rounds']} interleaved rounds; torch loss: {res['torch_loss']}; against torch float32: gradient "
             f"max diff / max {res['grad_rel_diff_to_torch']:.2e}, loss diff {res['loss_diff_to_torch']:.2e}",
             f"{'setting':<16}{'median ms':>11}{'min ms':>9}{'p90 ms':>9}{'GB/s moved':>12}{'x copy3':>9}{'x sub':>8}"
             f"{'x torch':>9}"]
    for name, e in res["settings"].items():
        lines.append(f"{name:<16}{e['median_ms']:>11}{e['min_ms']:>9}{e['p90_ms']:>9}{e.get('moved_GBps', ''):>12}"
                     f"{e['ratio_to_copy3']:>9}{e['ratio_to_sub']:>8}{e['ratio_to_torch']:>9}")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["1920x1080", "1600x1063"])
    ap.add_argument("--rounds", type=int, default=24)
    ap.add_argument("--warm-seconds", type=float, default=1.0)
    ap.add_argument("--label", default="", help="what to name in the report: the commit and the box")
    ap.add_argument("--out", default=None, help="also write the tables to this file")
    args = ap.parse_args()
    import torch
    results = [run_size(*map(int, s.lower().split("x")), args.rounds, args.warm_seconds) for s in args.sizes]
    head = f"tools/image_loss_bench.py  {args.label}  device: {torch.cuda.get_device_name(0)}"
    text = "\n\n".join([head] + [table(r) for r in results]) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(json.dumps({"label": args.label, "results": results}))


if __name__ == "__main__":
    main()
