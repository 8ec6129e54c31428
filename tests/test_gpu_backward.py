"""gsr_render_backward (Renderer.render_backward): the per-Gaussian gradients of the blend
against the float64 reference of tests/_backward_ref.py, which tests/test_backward_ref.py pins
to the unmodified oracle and to its own finite differences.

Error measure: |got - reference| / A per component and Gaussian, A the reference's scale
plane (the sum of the absolute values of the terms a gradient is made of).  Where A = 0 the
output must keep its prefilled value bit for bit.  The upstream gradient is zeroed at the
reference's ambiguous pixels on both sides."""
import numpy as np
import pytest

import _backward_ref as br

pytestmark = pytest.mark.gpu

# E32: the largest error / A of the SAME reference evaluated in float32 numpy, over every run
# of _backward_ref.RUNS (measured 7.10e-6, tests/test_backward_ref.py asserts the constant
# against the measurement).  The GPU tolerance is 8 E32: the factor covers a different exp,
# FMA contraction and the arbitrary order of the atomics.  It is measured against the
# reference, never against the kernel.
E32 = 7.5e-6
TOL = 8 * E32

KNOB_BLEND_EXP, KNOB_SPLIT, KNOB_PM, KNOB_STATE = 22, 23, 24, 26
ROWS = {"color": slice(0, 3), "opacity": slice(3, 4), "conic": slice(4, 8), "center": slice(8, 10)}
ALL = ("color", "opacity", "conic", "center")


@pytest.fixture(scope="module")
def torch(gpu):
    import torch as t
    assert t.cuda.is_available()
    return t


@pytest.fixture(scope="module")
def ref(gpu, orc, tmp_path_factory):
    return lambda case, g=(5, False, True, True): br.reference(gpu, orc, tmp_path_factory, case, g)


@pytest.fixture(scope="module")
def scene_of(gpu, orc, tmp_path_factory):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = gpu.Scene.from_soa(br.scenes(gpu, orc, tmp_path_factory)[name])
        return cache[name]
    return get


def tiling_of(gsr, case):
    c = br.CASES[case]
    if not c.get("tiling"):
        return None
    t = gsr.TilingInformation(1, 1, c["H"], c["W"])
    t.num_tile_x, t.num_tile_y, t.width_stride, t.height_stride = c["tiling"]
    return t


def device_g(torch, r):
    """The reference's upstream gradients (already zero at ambiguous pixels) on the device."""
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()  # noqa: E731
    return up(r["g_image"]), up(r["g_alpha"])


def new_block(torch, n, fill=0.0):
    """All ten planes as ONE (10, n) tensor, so a write outside a plane lands in a checked one."""
    return torch.full((10, n), fill, dtype=torch.float32, device="cuda")


def backward_into(gsr, r, scene, case, g_dev, block, what=ALL):
    """One complete backward frame of `case` into the planes `what` of block (accumulating): up
    to three renders until sync() == 0, the block put back ahead of each retry."""
    c = br.CASES[case]
    before = block.clone()
    ptr = {k: block[ROWS[k]].data_ptr() if k in what else None for k in ALL}
    for attempt in range(3):
        if attempt:
            block.copy_(before)
        r.render_backward(scene, br.camera(gsr, case), c["W"], c["H"], grad_image_ptr=g_dev[0], grad_alpha_ptr=g_dev[1],
                          color_ptr=ptr["color"], opacity_ptr=ptr["opacity"], conic_ptr=ptr["conic"],
                          center_ptr=ptr["center"], k=c.get("k", 3.0), tiling=tiling_of(gsr, case),
                          time=c.get("time"))
        if r.sync() == 0:
            return
    raise AssertionError("backward frame still incomplete after three renders")


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def assert_matches(block, refs, what=ALL, prefill=0.0, label=""):
    """Planes `what` of the (10, n) host block against the sum of the references `refs` (scales
    add); every other plane, and every entry with A = 0, keeps the prefill bit for bit."""
    worst = 0.0
    for kind in ALL:
        got = block[ROWS[kind]]
        if kind not in what:
            assert same_bits(got, np.full_like(got, prefill)), (label, kind, "not asked for, yet written")
            continue
        want = sum(r[kind].astype(np.float64) for r in refs)
        A = sum(r["A_" + kind] for r in refs)
        pos = A > 0
        err = np.abs(got.astype(np.float64) - prefill - want)[pos] / A[pos]
        print(label, kind, "worst error / A", float(err.max(initial=0.0)), "of", TOL)
        worst = max(worst, float(err.max(initial=0.0)))
        assert np.isfinite(got).all()
        assert same_bits(got[~pos], np.full_like(got[~pos], prefill)), (label, kind, "A = 0 entries changed")
        bad = np.argwhere((np.abs(got.astype(np.float64) - prefill - want) > TOL * A) & pos)
        assert len(bad) == 0, (label, kind, bad[:8], float(err.max()))
    assert worst > 0, (label, "nothing to compare")
    return worst


# ---------------------------------------------------------------- 1. all outputs, every run

@pytest.mark.parametrize("case,g", [(c, g) for c, g in br.RUNS if c != "overflow"])
def test_all_outputs_match_reference(gpu, torch, ref, scene_of, case, g):
    r = ref(case, g)
    assert r["takes"].sum() > 500 and br.mask_share(r) <= br.MASK_SHARE_CAP
    if case == "faint":
        assert r["takes"].max() > 300 and len(r["rec"]["order"]) == 3000
    block = new_block(torch, r["rec"]["n"])
    backward_into(gpu, gpu.Renderer(), scene_of(br.CASES[case]["scene"]), case, device_g(torch, r), block)
    assert_matches(block.cpu().numpy(), [r], label=f"{case} {g}")


# ---------------------------------------------------------------- 2. every subset of outputs

def test_every_subset_of_outputs(gpu, torch, ref, scene_of):
    r = ref("dense")
    g_dev = device_g(torch, r)
    rd = gpu.Renderer()
    for bits in range(1, 16):
        what = tuple(k for j, k in enumerate(ALL) if bits >> j & 1)
        block = new_block(torch, r["rec"]["n"], fill=-7.25)
        for k in what:
            block[ROWS[k]] = 0.0
        backward_into(gpu, rd, scene_of("dense"), "dense", g_dev, block, what)
        host = block.cpu().numpy()
        for k in ALL:
            if k not in what:
                assert same_bits(host[ROWS[k]], np.full_like(host[ROWS[k]], -7.25)), (what, k)
                host[ROWS[k]] = 0.0
        assert_matches(host, [r], what, label=str(what))


# ---------------------------------------------------------------- 3. untouched Gaussians

@pytest.mark.parametrize("case", ["dense", "dense99", "sparse_a"])
def test_uncomposited_gaussians_keep_their_value(gpu, orc, torch, ref, scene_of, case):
    """Gaussians no pixel composited (render_contrib's count of the same frame is 0: culled,
    off screen, or behind pixels that had all saturated) keep a prefilled 1.5 in every plane."""
    c = br.CASES[case]
    r = ref(case, next(g for name, g in br.RUNS if name == case))
    n = r["rec"]["n"]
    scene = scene_of(c["scene"])
    rd = gpu.Renderer()
    count = torch.zeros(n, dtype=torch.int32, device="cuda")
    for _ in range(3):
        rd.render_contrib(scene, br.camera(gpu, case), c["W"], c["H"], count_ptr=count.data_ptr())
        if rd.sync() == 0:
            break
    idle = count.cpu().numpy() == 0
    visible = np.zeros(n, bool)
    visible[r["rec"]["order"]] = True
    print(case, "never composited", int(idle.sum()), "of them visible", int((idle & visible).sum()))
    assert idle.sum() >= 4 and (~idle).sum() >= 50
    if case == "dense99":
        assert (idle & visible).sum() >= 5      # hidden behind saturated pixels: the alive exit ran
        assert (r["alpha"] > 0.999).sum() >= 500
    if case == "sparse_a":
        assert (idle & ~visible).sum() >= 100   # culled by the preprocess
    block = new_block(torch, n, fill=1.5)
    backward_into(gpu, rd, scene, case, device_g(torch, r), block)
    host = block.cpu().numpy()
    assert same_bits(host[:, idle], np.full_like(host[:, idle], 1.5))
    assert (host[0:4, ~idle] != 1.5).any(axis=0).mean() > 0.9    # and the others moved


# ---------------------------------------------------------------- 4. zero upstream gradient

def test_zero_gradient_changes_nothing(gpu, torch, ref, scene_of):
    r = ref("dense")
    c = br.CASES["dense"]
    block = torch.from_numpy(np.random.default_rng(3).standard_normal((10, r["rec"]["n"])).astype(np.float32)).cuda()
    before = block.cpu().numpy()
    zeros = (torch.zeros(3, c["H"], c["W"], device="cuda"), torch.zeros(c["H"], c["W"], device="cuda"))
    backward_into(gpu, gpu.Renderer(), scene_of("dense"), "dense", zeros, block)
    assert same_bits(block.cpu().numpy(), before)


# ---------------------------------------------------------------- 5. accumulation

def test_two_cameras_accumulate(gpu, torch, ref, scene_of):
    ra, rb = ref("sparse_a", (8, False, True, True)), ref("sparse_b", (9, False, True, True))
    block = new_block(torch, ra["rec"]["n"])
    rd = gpu.Renderer()
    backward_into(gpu, rd, scene_of("sparse"), "sparse_a", device_g(torch, ra), block)
    backward_into(gpu, rd, scene_of("sparse"), "sparse_b", device_g(torch, rb), block)
    only_a = (ra["A_color"][0] > 0) & ~(rb["A_color"][0] > 0)
    assert only_a.sum() > 50 and ((rb["A_color"][0] > 0) & ~(ra["A_color"][0] > 0)).sum() > 50
    assert_matches(block.cpu().numpy(), [ra, rb], label="two cameras")


# ---------------------------------------------------------------- 6. partial coverage
# (the dense_partial run of test_all_outputs_match_reference: its upstream gradient is
# non-zero outside the covered 60 x 40, and the reference ignores those pixels)

def test_partial_cover_case_has_gradient_outside(ref):
    r = ref("dense_partial", (11, False, True, True))
    assert np.abs(r["g_image"][:, 40:, :]).min() > 0 and np.abs(r["g_alpha"][:, 60:]).min() > 0
    assert not r["takes"][40:, :].any() and not r["takes"][:, 60:].any() and r["takes"].sum() > 1000
    full = ref("dense")
    assert full["count"].sum() > r["count"].sum() + 500     # the uncovered pixels would have composited


# ---------------------------------------------------------------- 7. overflow adds nothing

def test_overflow_frame_adds_nothing(gpu, torch, ref, scene_of):
    """tests/test_gpu_contrib.py's overflowing frame: the first render overflows the pair
    buffer and must leave the prefilled planes exactly as they were; the re-render is complete
    and matches the reference.  This frame cannot meet the mask-share condition, so its
    upstream gradient is confined to a few pixels (_backward_ref.CASES)."""
    case, g = "overflow", (14, False, True, True)
    c = br.CASES[case]
    r = ref(case, g)
    n = r["rec"]["n"]
    compared = ~r["mask"] & (r["takes"] > 0)
    print("pixels compared", int(compared.sum()), "takes up to", int(r["takes"].max()))
    assert compared.sum() >= 80 and r["takes"].max() > 200
    rd = gpu.Renderer()
    rd.reserve(n, 1024)
    g_dev = device_g(torch, r)
    block = new_block(torch, n, fill=1.5)
    kw = dict(grad_image_ptr=g_dev[0], grad_alpha_ptr=g_dev[1], color_ptr=block[ROWS["color"]].data_ptr(),
              opacity_ptr=block[ROWS["opacity"]].data_ptr(), conic_ptr=block[ROWS["conic"]].data_ptr(),
              center_ptr=block[ROWS["center"]].data_ptr())
    rd.render_backward(scene_of("overflow"), br.camera(gpu, case), c["W"], c["H"], **kw)
    assert rd.sync() == -5                      # overflow reported and buffer grown
    host = block.cpu().numpy()
    assert same_bits(host, np.full_like(host, 1.5))
    block.zero_()
    rd.render_backward(scene_of("overflow"), br.camera(gpu, case), c["W"], c["H"], **kw)
    assert rd.sync() == 0
    assert rd.pair_count() > 1_000_000
    assert_matches(block.cpu().numpy(), [r], label="overflow, re-rendered")


# ---------------------------------------------------------------- 8. 4D
# (the "4d" run of test_all_outputs_match_reference: _oracle.temporal at t = 0.3 on the
# reference side, time= on the GPU side, so the record's opacity is the temporal one)

def test_4d_case_has_temporal_opacity(gpu, orc, ref, tmp_path_factory):
    r = ref("4d", (12, False, True, True))
    soa49 = br.scenes(gpu, orc, tmp_path_factory)["4d"]
    assert soa49.shape[0] == 49
    vis = r["rec"]["order"]
    assert (np.abs(r["soa"][3, vis] - soa49[3, vis]) > 1e-3).sum() > 100    # the opacity moved with t


# ---------------------------------------------------------------- 9. frame policy

def plain(gsr, torch, scene, cam, W, H, renderer):
    out = torch.empty(3 * W * H, dtype=torch.float32, device="cuda")
    for _ in range(3):
        renderer.render(scene, cam, W, H, out.data_ptr())
        if renderer.sync() == 0:
            break
    return out.view(3, H, W).cpu().numpy()


def test_depth_split_controller_untouched(gpu, torch, ref, scene_of):
    case, g = "sparse_a", (8, False, True, True)
    c = br.CASES[case]
    r = ref(case, g)
    cam = br.camera(gpu, case)
    rd = gpu.Renderer()
    rd.set_tuning(KNOB_SPLIT, 1)
    rd.set_tuning(KNOB_PM, 150)
    for _ in range(2):
        plain(gpu, torch, scene_of("sparse"), cam, c["W"], c["H"], rd)
    before = (rd.get_tuning(KNOB_PM), rd.get_tuning(KNOB_STATE))
    block = new_block(torch, r["rec"]["n"])
    backward_into(gpu, rd, scene_of("sparse"), case, device_g(torch, r), block)
    assert (rd.get_tuning(KNOB_PM), rd.get_tuning(KNOB_STATE)) == before
    assert_matches(block.cpu().numpy(), [r], label="split on")


@pytest.mark.parametrize("blend_exp", [0, 1])
def test_exact_blend_whatever_the_knob(gpu, torch, ref, scene_of, blend_exp):
    r = ref("dense")
    rd = gpu.Renderer()
    rd.set_tuning(KNOB_BLEND_EXP, blend_exp)
    block = new_block(torch, r["rec"]["n"])
    backward_into(gpu, rd, scene_of("dense"), "dense", device_g(torch, r), block)
    assert rd.get_tuning(KNOB_BLEND_EXP) == blend_exp
    assert_matches(block.cpu().numpy(), [r], label=f"blend_exp {blend_exp}")


def test_next_plain_frame_is_unaffected(gpu, torch, ref, scene_of):
    """render, backward, render against render, render: the last frames are bit-identical."""
    case, g = "sparse_a", (8, False, True, True)
    c = br.CASES[case]
    r = ref(case, g)
    cam_a, cam_b = br.camera(gpu, "sparse_a"), br.camera(gpu, "sparse_b")
    ra, rb = gpu.Renderer(), gpu.Renderer()
    for rd in (ra, rb):
        plain(gpu, torch, scene_of("sparse"), cam_a, c["W"], c["H"], rd)
    block = new_block(torch, r["rec"]["n"])
    backward_into(gpu, ra, scene_of("sparse"), case, device_g(torch, r), block)
    last = [plain(gpu, torch, scene_of("sparse"), cam_b, c["W"], c["H"], rd) for rd in (ra, rb)]
    assert same_bits(last[0], last[1]) and last[0].any()
