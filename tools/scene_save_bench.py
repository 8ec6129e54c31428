#!/usr/bin/env python3
"""Cost of the scene export (Scene.pack_rows, Scene.save_ply; include/gsr.h "scene export")
against a device copy of the bytes the pack kernel must touch, against what a user had to do
before (Scene.download, a numpy de-activation and interleave, tofile) and against the I/O floor, a
bare write of the same byte count from pinned memory.  One process, interleaved as
tools/scene_init_bench.py does: after a warm-up every round runs each setting once, so clock,
thermal and page-cache drift hit all settings alike.

Per size (1M and 5M Gaussians, the sizes of configs 2 and 3; 38-array blocks, 62 floats a row):
  device settings, between two HIP events
    pack               Scene.pack_rows of the whole block into a device buffer, against
    copy_400n          a device copy of the 152 n bytes it reads + the 248 n it writes
  file settings, wall clock around the whole call, the file removed outside the timed span
    save               Scene.save_ply (default chunk), against
    numpy_today        Scene.download + numpy log / logit + interleave + ndarray.tofile, and
    pinned_write       os.write of the file's byte count from one pinned buffer
Checks at the timed sizes: the saved file equals write_ply(download()) byte for byte, and the
packed rows equal that file's rows.

    python tools/scene_save_bench.py [--sizes 1000000 5000000] [--rounds 20] [--file-rounds 5]
                                     [--dir DIR] [--label TEXT] [--out FILE]
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

ROW = 62   # floats per row of a 38-array block


def numpy_today(gsr, np, scene, path):
    """The exporter a user wrote before: download, undo the activations, interleave, write."""
    soa = scene.download()
    n = soa.shape[1]
    rows = np.zeros((n, ROW), np.float32)
    rows[:, 0:3] = soa[0:3].T
    rows[:, 6:9] = soa[11:14].T
    rows[:, 9:33] = soa[14:38].T
    o = soa[3]
    rows[:, 54] = np.log(o) - np.log1p(-o)
    rows[:, 55:58] = np.log(soa[4:7]).T
    rows[:, 58:62] = soa[7:11].T
    with open(path, "wb") as f:
        f.write(header(n))
        rows.tofile(f)


def header(n):
    names = ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"] + [f"f_rest_{j}" for j in range(45)] \
        + ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"]
    return ("ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % n
            + "".join(f"property float {p}\n" for p in names) + "end_header\n").encode()


def write_all(fd, view):
    while len(view):
        view = view[os.write(fd, view):]


def run_size(n, rounds, file_rounds, warm_seconds, d):
    import numpy as np
    import torch
    import gaussianrenderer_amd as gsr

    src = os.path.join(d, "src.ply")
    gsr.write_synthetic_ply(src, n, 1)
    scene = gsr.Scene.from_ply(src)
    os.remove(src)
    stream = torch.cuda.current_stream().cuda_stream
    packed = torch.empty(n * ROW, dtype=torch.float32, device="cuda")
    copy = [torch.empty(400 * n, dtype=torch.uint8, device="cuda") for _ in range(2)]
    file_bytes = len(header(n)) + 4 * ROW * n
    pinned = torch.empty(file_bytes, dtype=torch.uint8, pin_memory=True)
    pinned.fill_(1)
    path = os.path.join(d, "out.ply")

    def pinned_write():
        fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
        try:
            write_all(fd, memoryview(pinned.numpy()))
        finally:
            os.close(fd)

    # faster and different is not faster: the device's file and rows against the host writer's
    scene.save_ply(path)
    saved = open(path, "rb").read()
    ref = os.path.join(d, "ref.ply")
    gsr.write_ply(ref, scene.download())
    want = open(ref, "rb").read()
    os.remove(ref)
    file_equal = saved == want
    scene.pack_rows(packed, 0, n, stream=stream)
    torch.cuda.synchronize()
    rows_equal = packed.cpu().numpy().tobytes() == want[len(header(n)):]
    del saved, want

    device = [("pack", lambda: scene.pack_rows(packed, 0, n, stream=stream)),
              ("copy_400n", lambda: copy[1].copy_(copy[0]))]
    files = [("save", lambda: scene.save_ply(path)),
             ("numpy_today", lambda: numpy_today(gsr, np, scene, path)),
             ("pinned_write", pinned_write)]

    t0 = time.time()
    while time.time() - t0 < warm_seconds:
        for _, go in device:
            go()
        torch.cuda.synchronize()
    ms = {k: [] for k, _ in device + files}
    for _ in range(rounds):
        for k, go in device:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            go()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    for _ in range(file_rounds):
        for k, go in files:
            torch.cuda.synchronize()
            t = time.perf_counter()
            go()
            ms[k].append(1e3 * (time.perf_counter() - t))
            assert os.path.getsize(path) == file_bytes
            os.remove(path)

    rep = {}
    for k in ms:
        a = np.array(ms[k])
        rep[k] = {"median_ms": round(float(np.median(a)), 3), "min_ms": round(float(a.min()), 3),
                  "max_ms": round(float(a.max()), 3), "rounds": len(a)}
    rep["pack"]["GB_per_s"] = round(400 * n / rep["pack"]["median_ms"] / 1e6, 1)
    rep["copy_400n"]["GB_per_s"] = round(2 * 400 * n / rep["copy_400n"]["median_ms"] / 1e6, 1)
    for k in files:
        rep[k[0]]["GB_per_s"] = round(file_bytes / rep[k[0]]["median_ms"] / 1e6, 2)
    for k, against in (("pack", "copy_400n"), ("save", "numpy_today"), ("pinned_write", "save")):
        rep[k]["against"] = against
        rep[k]["ratio"] = round(rep[k]["median_ms"] / rep[against]["median_ms"], 3)
    scene.free()
    return {"n": n, "file_MB": round(file_bytes / 1e6, 1), "file_equals_host_writer": file_equal,
            "rows_equal_host_writer": rows_equal, "settings": rep}


def table(res):
    lines = [f"n = {res['n']:,}, file {res['file_MB']} MB; saved file == write_ply(download()): "
             f"{res['file_equals_host_writer']}; packed rows == its rows: {res['rows_equal_host_writer']}",
             f"{'setting':<14}{'median ms':>11}{'min ms':>11}{'max ms':>11}{'rounds':>8}{'GB/s':>9}   against"]
    for k, e in res["settings"].items():
        vs = f"   {e['ratio']} x {e['against']}" if "against" in e else ""
        lines.append(f"{k:<14}{e['median_ms']:>11}{e['min_ms']:>11}{e['max_ms']:>11}{e['rounds']:>8}{e['GB_per_s']:>9}{vs}")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[1_000_000, 5_000_000])
    ap.add_argument("--rounds", type=int, default=20, help="rounds of the device settings")
    ap.add_argument("--file-rounds", type=int, default=5, help="rounds of the file settings")
    ap.add_argument("--warm-seconds", type=float, default=1.0)
    ap.add_argument("--dir", default=None, help="where the files are written (default: a temporary directory)")
    ap.add_argument("--label", default="", help="what to name in the report: the commit and the box")
    ap.add_argument("--out", default=None, help="also write the tables to this file")
    args = ap.parse_args()
    import torch
    results = []
    with tempfile.TemporaryDirectory(dir=args.dir) as d:
        for n in args.sizes:
            results.append(run_size(n, args.rounds, args.file_rounds, args.warm_seconds, d))
    head = (f"tools/scene_save_bench.py  {args.label}  device: {torch.cuda.get_device_name(0)}\n"
            "GB/s: pack = (bytes read + written) / time; copy_400n = 2 x 400 n / time (a copy reads and writes "
            "each byte); file settings = file bytes / wall time (page cache included: no fsync)")
    text = "\n\n".join([head] + [table(r) for r in results]) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(json.dumps({"label": args.label, "results": results}))


if __name__ == "__main__":
    main()
