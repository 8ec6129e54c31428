"""Preconditions of tests/test_gpu_wide.py, on the CPU: the scenes of tests/_wide_scenes.py
reach the code the GPU tests are for.  Everything here is computed from the UNMODIFIED
oracle's records and images, never from the kernels or a restatement of them.  What a
(scene, camera, k) case reaches depends on its seed, so every floor is asserted per case."""
import numpy as np
import pytest

import _wide_scenes as ws
from test_gpu_parity import CAMS, cam_for, rect_pairs

W, H = ws.W, ws.H
TX, TY = (W + 15) // 16, (H + 15) // 16
CI = range(len(CAMS))

_cache = {}


def case(gsr, orc, name, ci, k=3.0):
    """The oracle's records of one case, once per module: the visible records, their tile
    rects and the number of rect pairs."""
    key = (name, ci, k)
    if key not in _cache:
        soa = ws.graze(int(name[5:])) if name.startswith("graze") else ws.scene(name)
        cam = cam_for(gsr, W, H, **CAMS[ci])
        want = orc.preprocess(soa, cam, W, H, k)
        x0, x1, y0, y1 = ws.tile_rects(want, W, H)
        pairs = ws.rect_pairs(want, orc.expected_depth_order(want), W, H)
        _cache[key] = dict(soa=soa, cam=cam, want=want, vis=want[want["status"] == 2], w=x1 - x0 + 1, h=y1 - y0 + 1,
                           pairs=pairs)
    return _cache[key]


def test_vectorised_rect_pairs_equal_the_loop(gsr, orc):
    for ci in CI:
        c = case(gsr, orc, "slabs", ci)
        order = orc.expected_depth_order(c["want"])
        slow = rect_pairs(c["want"], order, W, H)
        assert slow.size > 5000 and np.array_equal(c["pairs"], slow)
    # a rect that ends at W / H and one that starts at 0, at another k
    c = case(gsr, orc, "slabs", 0, 8.0)
    assert np.array_equal(c["pairs"], rect_pairs(c["want"], orc.expected_depth_order(c["want"]), W, H))


@pytest.mark.parametrize("ci", CI)
@pytest.mark.parametrize("name", ["slabs", "needles", "stack"])
def test_rects_wide_tall_and_across_the_frame(gsr, orc, name, ci):
    """Wider than six tiles (the spans' middle columns stay), taller than four tile rows (the
    rows past the fourth keep every column), and across the whole frame."""
    c = case(gsr, orc, name, ci)
    wide, tall = int((c["w"] > 6).sum()), int((c["h"] > 4).sum())
    across = int(((c["w"] == TX) | (c["h"] == TY)).sum())
    print(name, ci, "wider than 6 tiles", wide, "taller than 4 rows", tall, "all columns or rows", across)
    assert wide >= 40 and tall >= 80 and across >= 1


@pytest.mark.parametrize("ci", CI)
@pytest.mark.parametrize("name", ["slabs", "needles"])
def test_boxes_end_at_the_frame_and_centres_lie_outside(gsr, orc, name, ci):
    """aabb[2] == W and aabb[3] == H (ceilf of ndc 1.0: one past the last pixel), and visible
    splats whose centre pixel is off screen."""
    v = case(gsr, orc, name, ci)["vis"]
    right, bottom = int((v["aabb"][:, 2] == W).sum()), int((v["aabb"][:, 3] == H).sum())
    off = int(((v["px_x"] < 0) | (v["px_x"] >= W) | (v["px_y"] < 0) | (v["px_y"] >= H)).sum())
    print(name, ci, "aabb[2] == W", right, "aabb[3] == H", bottom, "off-screen centres", off)
    assert right >= 10 and bottom >= 10 and off >= 10
    a = v["aabb"]
    both = ((a[:, 0] == 0) & (a[:, 2] == W)) | ((a[:, 1] == 0) & (a[:, 3] == H))
    assert both.any()       # clamped on both sides of an axis


@pytest.mark.parametrize("seed", ws.GRAZE_SEEDS)
def test_graze_centres_far_off_screen(gsr, orc, seed):
    """Centres beyond +-8192 px (the spans' 1/64-px pad is argued for centres below 4096)."""
    c = case(gsr, orc, f"graze{seed}", 0)
    v = c["vis"]
    far = int(max(np.abs(v["px_x"].astype(np.int64)).max(), np.abs(v["px_y"].astype(np.int64)).max()))
    print("graze", seed, "visible", len(v), "largest |px|", far, "pairs", c["pairs"].size)
    assert far > 8192 and len(v) >= 150
    assert 80_000 <= c["pairs"].size <= 94_000 and c["pairs"].size < 120_000


@pytest.mark.parametrize("ci", CI)
def test_needles_straddle_the_robust_pd_test(gsr, orc, ci):
    """a e - h^2 > 1e-4 a e, the test below which the kernels give up their proofs."""
    ic = case(gsr, orc, "needles", ci)["vis"]["inv_covar"].astype(np.float32)
    a, b, c_, e = ic.T
    h = np.float32(0.5) * (b + c_)
    pd = (a * e - h * h) > np.float32(1e-4) * (a * e)
    print("needles", ci, "not robustly PD", int((~pd).sum()), "robustly PD", int(pd.sum()))
    assert (~pd).sum() >= 3 and pd.sum() >= 100


@pytest.mark.parametrize("ci", CI)
def test_stack_saturates_and_slabs_never_do(gsr, orc, ci):
    c = case(gsr, orc, "stack", ci)
    share = float((ws.alpha_plane(orc, c["soa"], c["cam"], W, H, 3.0) > 0.999).mean())
    print("stack", ci, "saturated share", share)
    assert share >= 0.60
    c = case(gsr, orc, "slabs", ci)
    assert not (ws.alpha_plane(orc, c["soa"], c["cam"], W, H, 3.0) > 0.999).any()


@pytest.mark.parametrize("ci", CI)
@pytest.mark.parametrize("name", ["slabs", "needles", "stack", "huge"])
def test_pair_counts_stay_small(gsr, orc, name, ci):
    """Hundreds of pairs per splat, yet few enough for the numpy side to stay at seconds."""
    p = case(gsr, orc, name, ci)["pairs"].size
    print(name, ci, "rect pairs", p)
    assert 5_000 <= p <= 76_000 and p < 120_000


def test_tilted_conics_have_off_diagonal_terms(gsr, orc):
    """What the identity-quaternion dense scenes lack: |b| comparable to sqrt(a e)."""
    soa = ws.scene("tilted")
    v = orc.preprocess(soa, cam_for(gsr, 128, 80), 128, 80, 3.0)
    ic = v[v["status"] == 2]["inv_covar"].astype(np.float64)
    r = np.abs(ic[:, 1]) / np.sqrt(ic[:, 0] * ic[:, 3])
    print("tilted: visible", len(ic), "median |b| / sqrt(a e)", float(np.median(r)))
    assert len(ic) >= 150 and np.median(r) > 0.2
