"""The 4D preprocess (k_preprocess<true, *>) on hand-made spacetime scenes
(tests/_temporal_scenes.py): its temporal cull at its boundary, its records, and the stages
behind it.

The 4D path has loads, arithmetic (the cubic motion, the temporal factor
gsr_expf(-(dt / trbf_scale)^2)) and a cull of its own: a Gaussian whose opacity at t is below
0.9e-3f and whose conic is robustly positive definite gets no record, because it provably
stays below alpha = 1e-3 on every pixel.  The reference has no such cull, so every expected
value here is the oracle's on orc.temporal(soa49, t), the 3D scene at time t, and the cull is
held to three statements: it is SOUND (what it drops cannot composite: opacity below 0.9e-3f
and a peak alpha below 1e-3f over the whole AABB, tests/test_temporal_scenes.py shows the same
on the reference side), it is THE DOCUMENTED ONE (the dropped set equals the predicate
evaluated in float32 on the oracle's record, so a low-opacity Gaussian that fails the PD test
keeps its record), and it DOES SOMETHING (at least a quarter of the visible Gaussians).
Everything else is the oracle's bit for bit: records (subnormal and NaN opacities included),
depth order, pair list, tile ranges, exact images, take maps in both blends.  320x240, k = 3,
test_gpu_parity.CAMS; tests/test_temporal_scenes.py asserts what the scenes reach."""
import os

import numpy as np
import pytest

import _temporal_scenes as ts
import _wide_scenes as ws
from conftest import exact_blend
from test_gpu_depth_split import KNOB_STATE, check_takes, split_renderer
from test_gpu_fastexp import take_parity
from test_gpu_parity import (CAMS, assert_image_parity, cam_for, check_preprocess_records, check_tile_spans,
                             max_alpha_on_tiles, render_gpu, same_opacity_bits, temporally_culled)
from test_gpu_path import render_path_checked
from test_temporal_scenes import RECORD_CASES, case

pytestmark = pytest.mark.gpu

W, H = ts.W, ts.H
ORC_THREADS = min(16, len(os.sched_getaffinity(0)))
KNOB_COMPACT = 18
BAND_SCENES = ("t_needles_band", "t_slabs_band")


@pytest.fixture(scope="module")
def torch(gpu):
    import torch as t
    assert t.cuda.is_available()
    return t


_frames, _gpu_scenes = {}, {}


def oracle_frame(orc, gpu, name, ci, t):
    """(image, take map) of one case from the oracle, computed once and left unchanged."""
    key = (name, ci, t)
    if key not in _frames:
        c = case(gpu, orc, name, ci, t)
        img, takes = orc.render_takes(c["soa3"], c["cam"], W, H, 3.0, threads=ORC_THREADS)
        img.setflags(write=False), takes.setflags(write=False)
        _frames[key] = (img, takes)
    return _frames[key]


def scene_of(gpu, name):
    if name not in _gpu_scenes:
        _gpu_scenes[name] = gpu.Scene.from_soa(ts.scene(name))
        assert _gpu_scenes[name].is_4d
    return _gpu_scenes[name]


def kept_order(orc, c):
    """The depth order of a 4D frame: the oracle's, with what the documented cull drops moved
    to key 0xFFFFFFFF."""
    return orc.expected_depth_order(ts.without(c["want"], c["culled"]))


# ---------------------------------------------------------------- a. records, order, lists

@pytest.mark.parametrize("name,ci,t", RECORD_CASES)
def test_records_order_and_lists_bit_exact(gpu, orc, name, ci, t):
    """Stage API at time t, spans off: every Gaussian the cull keeps has the oracle's record,
    key, tile_count and pairs; the cull is sound, is the documented predicate and is not idle."""
    c = case(gpu, orc, name, ci, t)
    r = gpu.Renderer()
    want = check_preprocess_records(gpu, orc, ts.scene(name), c["cam"], W, H, pairs_of=ws.rect_pairs, time=t,
                                    renderer=r)
    assert want.tobytes() == c["want"].tobytes()
    got = r.read_splats(want.shape[0])
    culled = temporally_culled(want, got)
    vis = c["vis"]
    # sound: nothing dropped could have composited
    assert (want["opacity"][culled] < ts.CULL_OPACITY).all()
    peak = max_alpha_on_tiles(want, ts.subset_pairs(orc, want, culled), W)
    share = culled.sum() / vis.sum()
    print(f"{name} camera {ci} t {t:g}: culled {int(culled.sum())} of {int(vis.sum())} visible ({share:.3f}), "
          f"their largest alpha {float(peak.max(initial=0.0)):.4e}; low & ~pd kept {int((c['low'] & ~c['pd']).sum())}")
    assert (peak < ts.TAKE_ALPHA).all()
    # the contract: exactly the documented predicate, so every low & ~pd Gaussian keeps its record
    wrong = np.nonzero(culled != c["culled"])[0]
    assert wrong.size == 0, (f"{wrong.size} Gaussians culled against the documented predicate, e.g. {wrong[:4].tolist()}: "
                             f"opacity {want['opacity'][wrong[:4]].tolist()}, conic {want['inv_covar'][wrong[:4]].tolist()}")
    assert (got["tile_count"][c["low"] & ~c["pd"]] > 0).all()
    if name in BAND_SCENES + ("t_slabs",):
        assert 4 * culled.sum() >= vis.sum()
    # the records hold the opacities the blend is to see, subnormals and NaN included
    kept = vis & ~culled
    # (a NaN's sign bit aside, which IEEE 754 leaves to the platform: same_opacity_bits)
    assert same_opacity_bits(got["opacity"][kept], c["soa3"][ts.A_OPACITY][kept], nan_sign_free=True)
    if name == "edges":
        nan = np.isnan(want["opacity"]) & kept
        tiny = kept & (want["opacity"] != 0) & (np.abs(want["opacity"]) < np.finfo(np.float32).tiny)
        print(f"edges camera {ci}: records with NaN opacity {int(nan.sum())}, subnormal {int(tiny.sum())}, "
              f"zero {int((kept & (want['opacity'] == 0)).sum())}")
        assert nan.sum() >= 16


# ---------------------------------------------------------------- b. the threshold itself

def test_threshold_to_the_bit(gpu, orc, torch):
    """boundary: dt = 0, so the opacity at t is the stored one bit for bit.  The eight Gaussians
    one float below 0.9e-3f are culled and no other; of the forty with a record, only the
    sixteen at or above 1e-3f composite (their centre pixel, once)."""
    t = ts.T0
    c = case(gpu, orc, "boundary", 0, t)
    scene = scene_of(gpu, "boundary")
    r = gpu.Renderer()
    r.preprocess(scene, c["cam"], W, H, time=t)
    r.sort()
    got = r.read_splats(48)
    assert np.array_equal(np.nonzero(got["tile_count"] == 0)[0], np.arange(8))
    assert (got["depth_key"][:8] == 0xFFFFFFFF).all() and (got["depth_key"][8:] != 0xFFFFFFFF).all()
    assert np.array_equal(got["opacity"][8:].view(np.uint32), ts.scene("boundary")[ts.A_OPACITY][8:].view(np.uint32))
    want, takes = oracle_frame(orc, gpu, "boundary", 0, t)
    linf, ce = take_parity(gpu, torch, scene, c["cam"], W, H, want, takes, mode=0, time=t)
    assert linf == 0.0 and ce["reblended_blocks"] == 0
    linf, _ = take_parity(gpu, torch, scene, c["cam"], W, H, want, takes, mode=1, time=t)
    print(f"boundary: fast-exp blend L-inf {linf:.3g}")
    count = torch.zeros(48, dtype=torch.int32, device="cuda")
    rc = gpu.Renderer()
    for _ in range(3):
        count.zero_()
        rc.render_contrib(scene, c["cam"], W, H, count_ptr=count.data_ptr(), time=t)
        if rc.sync() == 0:
            break
    else:
        raise AssertionError("contrib frame still incomplete after three renders")
    assert count.cpu().numpy().tolist() == [0] * 32 + [1] * 16


# ---------------------------------------------------------------- c. images and take maps, both blends

IMAGE_CASES = ([(s, ci, t) for s in ("t_slabs", "t_stack") for t in ts.TIMES for ci in (0, 2)]
               + [(s, ci, ts.T0) for s in BAND_SCENES for ci in (0, 2)]
               + [(s, ci, ts.T0) for s in ("edges", "edges_nan") for ci in (0, 2)])


@pytest.mark.parametrize("name,ci,t", IMAGE_CASES)
def test_take_maps_both_blends(gpu, orc, torch, name, ci, t):
    """The exact blend is bit-exact and re-blends nothing; the fast blend composites exactly
    the oracle's splats on every pixel, within FX_TOL.  edges_nan is the NaN-opacity group of
    edges on its own (alpha = fminf(NaN, 0.99): never culled, always composited)."""
    c = case(gpu, orc, name, ci, t)
    want, takes = oracle_frame(orc, gpu, name, ci, t)
    if name == "edges_nan":
        assert (takes & np.uint64(0xFFFFFFFF)).max() >= 1 and np.isfinite(want).all()
    scene = scene_of(gpu, name)
    linf, ce = take_parity(gpu, torch, scene, c["cam"], W, H, want, takes, mode=0, time=t)
    assert linf == 0.0 and ce["reblended_blocks"] == 0
    linf, cf = take_parity(gpu, torch, scene, c["cam"], W, H, want, takes, mode=1, time=t)
    print(f"{name} camera {ci} t {t:g}: fast-exp blend L-inf {linf:.3g}, re-blended blocks {cf['reblended_blocks']}, "
          f"most takes on a pixel {int((takes & np.uint64(0xFFFFFFFF)).max())}")


# ---------------------------------------------------------------- d. spans on 4D records

@pytest.mark.parametrize("name,ci", [(s, ci) for s in BAND_SCENES for ci in (0, 2)])
def test_tile_spans_on_4d_records(gpu, orc, torch, name, ci):
    """test_gpu_parity's spans test on records whose opacity lies around 1e-3 (in
    [0.9e-3, 1e-3) the md2 cut is negative): the spans-on list is a subsequence of the kept
    Gaussians' full list, every dropped pair peaks below 1e-3f, images are identical with
    spans on and off and equal the oracle's."""
    c = case(gpu, orc, name, ci, ts.T0)
    assert c["between"].sum() >= 8
    full, dropped, peak = check_tile_spans(gpu, orc, torch, ts.scene(name), c["cam"], W, H, floor=0.0,
                                           pairs_of=ws.rect_pairs, time=ts.T0)
    print(f"{name} camera {ci}: dropped share {dropped / full:.4f}, largest dropped alpha {peak:.4e}")
    assert dropped > 0


# ---------------------------------------------------------------- e. sort paths over a time sequence

SEQUENCE = (0.0, 0.7, -0.5, 0.4)


def sort_renderer(gpu, compact, buckets):
    r = exact_blend(gpu.Renderer())
    r.set_tuning(gpu.TUNE_DEPTH_SPLIT, 0)
    r.set_tuning(KNOB_COMPACT, compact)
    r.set_tuning(gpu.TUNE_DEPTH_BUCKETS, buckets)
    return r


@pytest.mark.parametrize("buckets", [0, 1])
@pytest.mark.parametrize("compact", [0, 1, 2])
def test_sort_paths_over_a_time_sequence(gpu, orc, torch, compact, buckets):
    """t_slabs at four times in sequence on one context (the culled set changes by about half
    from frame to frame; 0.4 is no time of the other tests): after every frame the depth order
    is the oracle's with the culled Gaussians last, the pair list is the unpartitioned LSD
    context's and the image the oracle's."""
    scene = scene_of(gpu, "t_slabs")
    n = scene.n
    r, base = sort_renderer(gpu, compact, buckets), sort_renderer(gpu, 0, 0)
    before = None
    for t in SEQUENCE:
        c = case(gpu, orc, "t_slabs", 0, t)
        if before is not None:
            print(f"t {t:g}: culled {int(c['culled'].sum())}, {int((c['culled'] != before).sum())} changed")
            assert (c["culled"] != before).sum() >= n // 4
        before = c["culled"]
        img, _ = render_gpu(gpu, torch, scene, c["cam"], W, H, renderer=r, time=t)
        render_gpu(gpu, torch, scene, c["cam"], W, H, renderer=base, time=t)
        assert np.array_equal(r.read_depth_order(n), kept_order(orc, c)), f"depth order at t {t:g}"
        pairs = r.read_pairs()
        assert pairs.size > 100 and np.array_equal(pairs, base.read_pairs()), f"pair list at t {t:g}"
        assert_image_parity(img, oracle_frame(orc, gpu, "t_slabs", 0, t)[0], exact=True)
    r.close(), base.close()


# ---------------------------------------------------------------- f. forced depth split

@pytest.mark.parametrize("pm", [50, 500])
def test_forced_depth_split(gpu, orc, torch, pm):
    """t_stack, camera 1, the split forced at 5 % and 50 % of the depth order, three frames at
    times 0.3, 0.3 and 0.7: count mode first, then the depth threshold of the frame before
    (which, for the third, is another time's).  Each exact, with the oracle's take map."""
    scene = scene_of(gpu, "t_stack")
    r = split_renderer(gpu, 1, pm)
    out = torch.empty(3 * W * H, dtype=torch.float32, device="cuda")
    for i, t in enumerate((0.3, 0.3, 0.7)):
        c = case(gpu, orc, "t_stack", 1, t)
        want, takes = oracle_frame(orc, gpu, "t_stack", 1, t)
        for attempt in range(3):            # rendered again on GSR_E_OVERFLOW, as render_gpu does
            r.render(scene, c["cam"], W, H, out.data_ptr(), time=t)
            rc = r.sync()
            state = r.get_tuning(KNOB_STATE)
            print(f"t_stack split at {pm / 10:g} %, frame {i} t {t:g}, attempt {attempt}: state {state}, sync {rc}")
            assert state == 1 if (i == 0 and attempt == 0) else state in (2, 3)
            if rc == 0:
                break
        assert_image_parity(out.view(3, H, W).cpu().numpy(), want, exact=True)
        check_takes(gpu, torch, r, scene, c["cam"], W, H, want, takes, time=t)
    r.close()


# ---------------------------------------------------------------- g. path

@pytest.mark.parametrize("exact", [True, False])
def test_render_path_over_cameras_and_times(gpu, orc, torch, exact):
    """gsr_render_path, four frames in flight, eight frames of t_slabs over the four cameras
    and the five times: each frame equals a single render of it bit for bit and the oracle's
    by its blend's rule."""
    scene = scene_of(gpu, "t_slabs")
    cis = [i % len(CAMS) for i in range(8)]
    times = [ts.TIMES[i % len(ts.TIMES)] for i in range(8)]
    cams = [cam_for(gpu, W, H, **CAMS[ci]) for ci in cis]
    r = gpu.Renderer()
    r.set_frames_in_flight(4)
    r.set_tuning(22, 0 if exact else 1)
    outs = [torch.full((3 * W * H,), -1.0, device="cuda") for _ in cams]
    render_path_checked(r, scene, cams, W, H, [o.data_ptr() for o in outs], times=times)
    for i, (ci, t) in enumerate(zip(cis, times)):
        got = outs[i].view(3, H, W).cpu().numpy()
        one = gpu.Renderer()
        one.set_tuning(22, 0 if exact else 1)
        single, _ = render_gpu(gpu, torch, scene, cams[i], W, H, renderer=one, time=t)
        assert np.array_equal(got.view(np.uint32), single.view(np.uint32)), f"frame {i}: path vs plain render"
        assert_image_parity(got, oracle_frame(orc, gpu, "t_slabs", ci, t)[0], exact=exact)


# ---------------------------------------------------------------- h. backward sees nothing of a culled Gaussian

def test_backward_leaves_culled_gaussians_alone(gpu, orc, torch):
    """gsr_render_backward on t_slabs_band: a temporally culled Gaussian has no pair, so no
    pixel hands it a gradient: all ten planes keep a prefilled 1.5 bit for bit."""
    t = ts.T0
    c = case(gpu, orc, "t_slabs_band", 0, t)
    scene = scene_of(gpu, "t_slabs_band")
    n = scene.n
    culled = c["culled"]
    assert culled.sum() >= 90
    g = torch.Generator(device="cpu").manual_seed(7)
    g_img = torch.randn(3, H, W, generator=g).cuda()
    g_alpha = torch.randn(H, W, generator=g).cuda()
    r = gpu.Renderer()
    for _ in range(3):
        block = torch.full((10, n), 1.5, dtype=torch.float32, device="cuda")   # one tensor: colour 3, opacity 1, conic 4, centre 2
        r.render_backward(scene, c["cam"], W, H, grad_image_ptr=g_img, grad_alpha_ptr=g_alpha, color_ptr=block[0:3],
                          opacity_ptr=block[3], conic_ptr=block[4:8], center_ptr=block[8:10], time=t)
        if r.sync() == 0:
            break
    else:
        raise AssertionError("backward frame still incomplete after three renders")
    host = block.cpu().numpy()
    assert np.array_equal(host[:, culled].view(np.uint32), np.full_like(host[:, culled], 1.5).view(np.uint32))
    moved = (host[:, ~culled] != 1.5).any(axis=0)
    print(f"t_slabs_band backward: {int(culled.sum())} culled untouched, {int(moved.sum())} of {int((~culled).sum())} others moved")
    assert moved.sum() >= 50
