"""bench.py as the driver runs it: a plain run prints the headline line only (no
--full objects) and --dump-outputs writes the last timed frame, which must be the
oracle's render of the bench scene and camera."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, assert_frames

pytestmark = pytest.mark.gpu


def test_plain_run_dumps_last_timed_frame(gpu, orc, tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    from gaussianrenderer_amd import multi
    n, W, H, seed = bench.CONFIGS[1]
    dump = tmp_path / "dump"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "1",
                          "--steps", "7", "--warmup", "2", "--warm-ms", "50", "--scene-dir", str(tmp_path),
                          "--dump-outputs", str(dump)],
                         capture_output=True, text=True, timeout=110)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    res = lines[0]
    assert res["steps"] == 7 and res["full"] is False and res["unit"] == "frames/sec"
    assert res["ms_per_step"] > 0 and res["value"] == pytest.approx(1e3 / res["ms_per_step"], rel=1e-3)
    for key in ("sequential", "roofline", "stages_ms", "cpu_baseline", "sh3", "orbit", "dropin_host_fps"):
        assert key not in res
    assert sorted(os.listdir(dump)) == ["image.npy"]
    got = np.load(dump / "image.npy")
    assert got.dtype == np.float32 and got.shape == (3, H, W)
    ply = tmp_path / f"config1_n{n}_s{seed}.ply"
    want = orc.render(gpu.read_ply(str(ply)), multi.orbit_camera(0, W, H), W, H, 3.0)
    assert (want != 0).sum() > 1000
    assert_frames(got, want.reshape(3, H, W))
