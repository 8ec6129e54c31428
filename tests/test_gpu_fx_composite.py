"""The fast-exp blend's compositing loop at its edges, against the oracle.

The fast loop (gsr_blend.hip, `blend_block` with FX) takes a batch's survivors two at a time
from 32 pair slots, forms each composite's weight alpha * T once for the three channels and
computes a pair's T-independent part one pair ahead of its transmittance chain.  The scenes
here are the smallest that reach what can go wrong there: odd and even survivor counts (the
unused half-slot), full batches (slot 31 has no successor) and the batch edge, pixels that
saturate on the first and on the second splat of a pair, lanes that take neither splat of a
pair, partial blocks and padding lanes, and records that send a block to the exact re-blend.

Every case checks, on images of at most 64x48 unless stated: the fast blend (knob 22 = 1,
depth split off) within 1e-5 of the oracle with the oracle's take map, its diagnostics frame
bit-equal to the plain one, and the exact blend (22 = 0) bit-equal to the oracle."""
import os

import numpy as np
import pytest

import _wide_scenes as ws
from conftest import KNOB_BLEND_EXP
from test_gpu_parity import CAMS, cam_for, render_gpu

pytestmark = pytest.mark.gpu

KNOB_DEPTH_SPLIT = 23
FX_BOUND = 1e-5
ORC_THREADS = min(16, len(os.sched_getaffinity(0)))
W, H = 64, 48
# pixels per world unit at the default camera's distance 4 (fov 50): (H / 2) / tan(25 deg) / 4
PX = 24.0 / np.tan(np.radians(25.0)) / 4.0


@pytest.fixture(scope="module")
def torch(gpu):
    import torch as t
    assert t.cuda.is_available()
    return t


def frames(gpu, torch, scene, cam, W, H, mode):
    """(image, diagnostics image, take map, counters) of one blend mode."""
    r = gpu.Renderer()
    r.set_tuning(KNOB_BLEND_EXP, mode)
    r.set_tuning(KNOB_DEPTH_SPLIT, 0)
    img, _ = render_gpu(gpu, torch, scene, cam, W, H, renderer=r)
    r.set_diagnostics(True)
    img_d, _ = render_gpu(gpu, torch, scene, cam, W, H, renderer=r)
    takes = r.take_map(W, H)
    counters = r.blend_counters_ex()
    r.set_diagnostics(False)
    return img, img_d, takes, counters


def composite_parity(gpu, orc, torch, soa, W=W, H=H, cam=None, sh3=False):
    """The four checks of this file on one scene; returns (oracle take counts, fast counters)."""
    cam = cam or cam_for(gpu, W, H)
    if sh3:
        with orc.sh3_mode():
            want, takes_want = orc.render_takes(soa, cam, W, H, 3.0, threads=ORC_THREADS)
    else:
        want, takes_want = orc.render_takes(soa, cam, W, H, 3.0, threads=ORC_THREADS)
    scene = gpu.Scene.from_soa(soa)
    finite = np.isfinite(want)
    for mode in (1, 0):
        img, img_d, takes, counters = frames(gpu, torch, scene, cam, W, H, mode)
        assert np.array_equal(img.view(np.uint32), img_d.view(np.uint32)), f"mode {mode}: diagnostics frame differs"
        bad = takes != takes_want
        assert not bad.any(), (f"mode {mode}: {int(bad.sum())} pixels composited other splats, e.g. "
                               f"{np.argwhere(bad)[:3].tolist()}: {takes[bad][:3]} vs {takes_want[bad][:3]}")
        # a non-finite colour (the re-blend case) must come out as the oracle's, bit for bit
        assert np.array_equal(img.view(np.uint32)[~finite], want.view(np.uint32)[~finite])
        if mode == 1:
            linf = float(np.abs(img[finite].astype(np.float64) - want[finite].astype(np.float64)).max())
            print(f"fast blend L-inf {linf:.3g}, re-blended blocks {counters['reblended_blocks']}")
            assert linf < FX_BOUND
            fast_counters = counters
        else:
            assert np.array_equal(img.view(np.uint32), want.view(np.uint32)), "exact blend not bit-equal"
    return (takes_want & np.uint64(0xFFFFFFFF)).astype(np.int64), fast_counters


def splats(rng, x_px, y_px, sigma_px, opacity, narrays=38):
    """Isotropic splats at z = 0 whose centres lie (x_px, y_px) pixels from the image centre
    (64x48, default camera) with a footprint of sigma_px pixels, in index = depth order
    (equal depths: the sort is stable), random colours."""
    n = len(opacity)
    soa = np.zeros((narrays, n), np.float32)
    soa[0] = np.asarray(x_px, np.float64) / PX
    soa[1] = np.asarray(y_px, np.float64) / PX
    soa[3] = opacity
    soa[4:7] = np.asarray(sigma_px, np.float64) / PX
    soa[7] = 1.0
    soa[11:14] = rng.normal(0.0, 1.5, (3, n))
    if narrays == 38:
        soa[14:38] = rng.normal(0.0, 0.3, (24, n))
    return soa


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 129])
def test_identical_footprints(gpu, orc, torch, n):
    """n splats of one footprint over one block, faint enough that no pixel saturates: every
    batch of the block holds min(64, what is left) survivors, so the counts cover the unused
    half-slot (odd), a full batch whose pair 31 has no successor (64, 65, 129) and a last
    pair that is not the slot's last."""
    rng = np.random.default_rng(100 + n)
    soa = splats(rng, np.full(n, -4.0), np.full(n, -4.0), 1.5, rng.uniform(0.005, 0.04, n))
    counts, c = composite_parity(gpu, orc, torch, soa)
    assert counts.max() == n          # some pixel composited all of them
    assert c["reblended_blocks"] == 0


@pytest.mark.parametrize("lead", [0, 1])
def test_saturating_stacks(gpu, orc, torch, lead):
    """Opacity-1.0 splats behind `lead` faint ones: near the centre T falls below 1e-3 on the
    second opaque splat, which is the second splat of a pair for lead = 0 and the first for
    lead = 1; further out it takes more.  The splats after a pixel's saturation add nothing."""
    rng = np.random.default_rng(200 + lead)
    n = 12
    op = np.concatenate([np.full(lead, 0.3), np.ones(n - lead)])
    soa = splats(rng, np.full(n, -4.0), np.full(n, -4.0), 4.0, op)
    counts, _ = composite_parity(gpu, orc, torch, soa)
    stopped = counts[(counts > 0) & (counts < n)]          # saturated before the list's end
    assert (stopped % 2 == 0).any() and (stopped % 2 == 1).any()
    assert stopped.min() == 2 + lead


def test_disjoint_boxes(gpu, orc, torch):
    """Small splats in turn at the four corners of one block: their boxes are disjoint, so in
    every pair most lanes take neither splat and no lane takes both."""
    rng = np.random.default_rng(300)
    n = 24
    x = np.tile([-7.0, -2.0, -7.0, -2.0], n // 4)
    y = np.tile([-7.0, -7.0, -2.0, -2.0], n // 4)
    soa = splats(rng, x, y, 0.5, rng.uniform(0.2, 0.9, n))
    counts, _ = composite_parity(gpu, orc, torch, soa)
    assert 3 <= counts.max() <= n // 4
    assert (counts == 0).sum() > W * H - 4 * 25             # each corner's box is at most 5x5


@pytest.mark.parametrize("W,H", [(37, 23), (17, 300)])
def test_partial_blocks(gpu, orc, torch, W, H):
    """Image sizes that are no multiple of the block: partial blocks and padding lanes."""
    soa = ws.unit_opacity(ws.scene("tilted"))
    counts, _ = composite_parity(gpu, orc, torch, soa, W, H)
    assert counts.max() > 3


@pytest.mark.parametrize("what", ["colour", "opacity"])
def test_record_without_fast_proof(gpu, orc, torch, what):
    """One record of an otherwise fast batch has a non-finite colour (an SH-3 scene, whose
    colour is not clamped above: f_dc = +inf) or an opacity above 1: the fast pass gives the
    block up and the exact re-blend composites it, bit for bit where the colour is infinite."""
    rng = np.random.default_rng(400)
    n = 21
    narrays = 59 if what == "colour" else 38
    soa = splats(rng, np.full(n, -4.0), np.full(n, -4.0), 1.5, rng.uniform(0.02, 0.2, n), narrays)
    if what == "colour":
        soa[11, 7] = np.inf
    else:
        soa[3, 7] = 1.3
    counts, c = composite_parity(gpu, orc, torch, soa, sh3=what == "colour")
    assert counts.max() > 7
    assert c["reblended_blocks"] > 0


@pytest.mark.parametrize("ci", [0, 1])
def test_random_scene(gpu, orc, torch, ci):
    """200 random tilted splats (tests/_wide_scenes.py), opacities capped at 1 so that the fast
    blend's own arithmetic composites them, on two cameras."""
    soa = ws.unit_opacity(ws.scene("tilted"))
    counts, _ = composite_parity(gpu, orc, torch, soa, cam=cam_for(gpu, W, H, **CAMS[ci]))
    assert counts.max() > 3
