"""gsr_project_backward and gsr_render_backward_scene (Renderer.project_backward,
Renderer.render_backward_scene): the gradients with respect to the scene arrays against the
float64 torch.autograd reference of tests/_project_ref.py, which tests/test_project_ref.py pins
to the unmodified oracle and to its own central differences.

Error measure: |got - reference| / A per output plane and Gaussian, A the reference's per-group
scale.  Where A = 0, and at every skipped Gaussian, the output keeps its prefilled value bit for
bit.  The upstream is standard normal on ALL n Gaussians (the off-screen and the culled ones
too) and zeroed on both sides at the reference's ambiguous Gaussians."""
import numpy as np
import pytest

import _backward_ref as br
import _project_ref as pr

pytestmark = pytest.mark.gpu

# E32: the largest error / A of the SAME reference evaluated in float32 torch, over every case
# of _project_ref.CASES (measured 7.5e-5, at a Gaussian 0.2 in front of sparse_in's camera;
# tests/test_project_ref.py asserts the constant against the measurement).  The GPU tolerance is
# 8 E32: the factor covers another operation order and the device's division and sqrt.  It is
# measured against the reference, never against the kernel.
E32 = 8.0e-5
TOL = 8 * E32

KNOB_SPLIT, KNOB_PM, KNOB_STATE = 23, 24, 26
INPUTS = ("color", "opacity", "conic", "center")


@pytest.fixture(scope="module")
def torch(gpu):
    import torch as t
    assert t.cuda.is_available()
    return t


@pytest.fixture(scope="module")
def ref(gpu, tmp_path_factory):
    return lambda case: pr.reference(gpu, tmp_path_factory, case)


@pytest.fixture(scope="module")
def scene_of(gpu, tmp_path_factory):
    cache = {}

    def get(case):
        if case not in cache:
            cache[case] = gpu.Scene.from_soa(pr.case_soa(gpu, tmp_path_factory, case))
        return cache[case]
    return get


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def new_block(torch, narrays, n, fill=0.0):
    """All output planes as ONE (narrays, n) tensor in the scene block's array order, so that a
    write outside a plane lands in a checked one."""
    return torch.full((narrays, n), fill, dtype=torch.float32, device="cuda")


def out_ptrs(block, what=None):
    g = pr.groups(block.shape[0])
    return {name + "_ptr": block[rows].data_ptr() if what is None or name in what else None
            for name, rows in g.items()}


def in_ptrs(up, which=INPUTS):
    return {"d_" + name + "_ptr": up[pr.REC_ROWS[name]].data_ptr() if name in which else None for name in INPUTS}


def project(gsr, torch, rd, scene, case, up, block, what=None, which=INPUTS, cases=pr.CASES, camera=pr.camera):
    c = cases[case]
    rd.project_backward(scene, camera(gsr, case), c["W"], c["H"], **in_ptrs(up, which), **out_ptrs(block, what),
                        k=c.get("k", 3.0), time=c.get("time"))
    torch.cuda.synchronize()


def assert_matches(host, refs, what=None, prefill=0.0, label=""):
    """The (narrays, n) host block against the sum of the references `refs` (their scales add):
    groups in `what` within TOL A where A > 0 and bit-identical to the prefill where A = 0;
    groups not asked for keep the prefill bit for bit."""
    worst, compared = 0.0, 0
    for name, rows in pr.groups(host.shape[0]).items():
        got = host[rows]
        if what is not None and name not in what:
            assert same_bits(got, np.full_like(got, prefill)), (label, name, "not asked for, yet written")
            continue
        want = sum(r["grad"][rows] for r in refs)
        A = sum(r["A"][rows] for r in refs)
        pos = A > 0
        compared += int(pos.sum())
        assert np.isfinite(got).all()
        err = np.abs(got.astype(np.float64) - prefill - want)[pos] / A[pos]
        print(label, name, "worst error / A", float(err.max(initial=0.0)), "of", TOL)
        worst = max(worst, float(err.max(initial=0.0)))
        assert same_bits(got[~pos], np.full_like(got[~pos], prefill)), (label, name, "A = 0 entries changed")
        bad = np.argwhere((np.abs(got.astype(np.float64) - prefill - want) > TOL * A) & pos)
        assert len(bad) == 0, (label, name, bad[:8], float(err.max()))
    assert compared > 0, (label, "nothing to compare")      # (the opacity alone matches exactly: worst = 0)
    return worst


# ---------------------------------------------------------------- 1. all outputs, every case

@pytest.mark.parametrize("case", list(pr.CASES))
def test_all_outputs_match_reference(gpu, torch, ref, scene_of, case):
    r = ref(case)
    narrays, n = r["soa"].shape
    assert pr.ambiguous_share(r) <= pr.AMBIGUOUS_SHARE_CAP
    if case == "sparse_in":
        assert (~r["valid"]).sum() >= 100
    up = torch.from_numpy(np.array(r["upstream"])).cuda()
    rd = gpu.Renderer()
    block = new_block(torch, narrays, n)
    project(gpu, torch, rd, scene_of(case), case, up, block)
    host = block.cpu().numpy()
    assert_matches(host, [r], label=case)
    # a prefilled block keeps its bits where A = 0 and at every skipped Gaussian
    block = new_block(torch, narrays, n, fill=1.5)
    project(gpu, torch, rd, scene_of(case), case, up, block)
    filled = block.cpu().numpy()
    skipped = ~r["valid"] | ~r["upstream"].any(0)
    keep = (r["A"] == 0) | skipped[None]
    assert same_bits(filled[keep], np.full_like(filled[keep], 1.5))
    assert (filled[:, ~skipped] != 1.5).any(axis=0).all()      # and every other Gaussian moved


# ---------------------------------------------------------------- 2. subsets of outputs and inputs

@pytest.mark.parametrize("case", ["rot", "4d"])
def test_each_group_and_each_input_alone(gpu, torch, ref, scene_of, tmp_path_factory, case):
    c = pr.CASES[case]
    r = ref(case)
    narrays, n = r["soa"].shape
    up = torch.from_numpy(np.array(r["upstream"])).cuda()
    rd = gpu.Renderer()
    for name in pr.groups(narrays):                       # one output group, every input
        block = new_block(torch, narrays, n, fill=-7.25)
        block[pr.groups(narrays)[name]] = 0.0
        project(gpu, torch, rd, scene_of(case), case, up, block, what=(name,))
        host = block.cpu().numpy()
        for other, rows in pr.groups(narrays).items():
            if other != name:
                assert same_bits(host[rows], np.full_like(host[rows], -7.25)), (name, other)
                host[rows] = 0.0
        assert_matches(host, [r], what=(name,), label=f"{case} only {name}")
    for name in INPUTS:                                   # one input plane group, every output
        only = np.zeros_like(r["upstream"])
        only[pr.REC_ROWS[name]] = r["upstream"][pr.REC_ROWS[name]]
        one = pr.evaluate(r["soa"], r["camv"], c["W"], c["H"], c.get("time", 0.0), upstream=only, valid=r["valid"])
        one["A"] = pr.scale(one["abs"], narrays)
        block = new_block(torch, narrays, n)
        project(gpu, torch, rd, scene_of(case), case, up, block, which=(name,))
        assert_matches(block.cpu().numpy(), [one], label=f"{case} input {name} alone")


# ---------------------------------------------------------------- 3. skipped Gaussians

def test_skipped_gaussians_keep_their_value(gpu, torch, ref, scene_of):
    case = "sparse_in"
    r = ref(case)
    narrays, n = r["soa"].shape
    upstream = np.array(r["upstream"])
    zeroed = np.random.default_rng(5).random(n) < 1 / 3
    upstream[:, zeroed] = 0.0
    invalid_live = ~r["valid"] & upstream.any(0)
    valid_zero = r["valid"] & ~upstream.any(0)
    rest = r["valid"] & upstream.any(0)
    print("invalid with upstream", int(invalid_live.sum()), "valid without", int(valid_zero.sum()), "rest", int(rest.sum()))
    assert invalid_live.sum() >= 100 and valid_zero.sum() >= 100 and rest.sum() >= 500
    block = new_block(torch, narrays, n, fill=1.5)
    project(gpu, torch, gpu.Renderer(), scene_of(case), case, torch.from_numpy(upstream).cuda(), block)
    host = block.cpu().numpy()
    assert same_bits(host[:, invalid_live], np.full_like(host[:, invalid_live], 1.5))
    assert same_bits(host[:, valid_zero], np.full_like(host[:, valid_zero], 1.5))
    assert (host[:, rest] != 1.5).any(axis=0).mean() > 0.9


# ---------------------------------------------------------------- 4. accumulation

def test_two_cameras_accumulate(gpu, torch, ref, scene_of):
    ra, rb = ref("sparse_a"), ref("sparse_b")
    narrays, n = ra["soa"].shape
    block = new_block(torch, narrays, n)
    rd = gpu.Renderer()
    project(gpu, torch, rd, scene_of("sparse_a"), "sparse_a", torch.from_numpy(np.array(ra["upstream"])).cuda(), block)
    project(gpu, torch, rd, scene_of("sparse_a"), "sparse_b", torch.from_numpy(np.array(rb["upstream"])).cuda(), block)
    assert_matches(block.cpu().numpy(), [ra, rb], label="two cameras")


# ---------------------------------------------------------------- 5. determinism

@pytest.mark.parametrize("case", ["sparse_in", "4d"])
def test_two_calls_give_identical_bits(gpu, torch, ref, scene_of, case):
    r = ref(case)
    narrays, n = r["soa"].shape
    up = torch.from_numpy(np.array(r["upstream"])).cuda()
    hosts = []
    for _ in range(2):
        block = new_block(torch, narrays, n)
        project(gpu, torch, gpu.Renderer(), scene_of(case), case, up, block)
        hosts.append(block.cpu().numpy())
    assert same_bits(hosts[0], hosts[1]) and hosts[0].any()


# ---------------------------------------------------------------- 6. the context is left alone

def plain(gsr, torch, scene, cam, W, H, renderer):
    out = torch.empty(3 * W * H, dtype=torch.float32, device="cuda")
    for _ in range(3):
        renderer.render(scene, cam, W, H, out.data_ptr())
        if renderer.sync() == 0:
            break
    return out.view(3, H, W).cpu().numpy()


def test_context_untouched(gpu, torch, ref, scene_of):
    """render, project_backward (another camera), read_splats, render against render,
    read_splats, render: the readbacks and the last frames are bit-identical."""
    r = ref("sparse_b")
    narrays, n = r["soa"].shape
    c = pr.CASES["sparse_a"]
    cam_a, cam_in = pr.camera(gpu, "sparse_a"), pr.camera(gpu, "sparse_in")
    ra, rb = gpu.Renderer(), gpu.Renderer()
    for rd in (ra, rb):
        plain(gpu, torch, scene_of("sparse_a"), cam_a, c["W"], c["H"], rd)
    block = new_block(torch, narrays, n)
    project(gpu, torch, ra, scene_of("sparse_a"), "sparse_b", torch.from_numpy(np.array(r["upstream"])).cuda(), block)
    assert block.any()
    splats = [rd.read_splats(n) for rd in (ra, rb)]
    # (a culled Gaussian's record is never written: its bytes are whatever the workspace held)
    assert np.array_equal(splats[0]["depth_key"], splats[1]["depth_key"])
    vis = splats[0]["depth_key"] != 0xFFFFFFFF
    assert vis.sum() > 1000 and splats[0][vis].tobytes() == splats[1][vis].tobytes()
    last = [plain(gpu, torch, scene_of("sparse_a"), cam_in, c["W"], c["H"], rd) for rd in (ra, rb)]
    assert same_bits(last[0], last[1]) and last[0].any()


# ---------------------------------------------------------------- 7-9. the fused call

@pytest.fixture(scope="module")
def bref(gpu, orc, tmp_path_factory):
    return lambda case: br.reference(gpu, orc, tmp_path_factory, case, next(g for name, g in br.RUNS if name == case))


@pytest.fixture(scope="module")
def bscene_of(gpu, orc, tmp_path_factory):
    cache = {}

    def get(name):
        if name not in cache:
            soa = br.scenes(gpu, orc, tmp_path_factory)[name]
            cache[name] = (soa, gpu.Scene.from_soa(soa))
        return cache[name]
    return get


def fused(gsr, torch, rd, scene, case, g_dev, scratch, block, retries=3):
    """One complete fused frame of _backward_ref's `case` into block (accumulating): up to
    `retries` renders until sync() == 0, the block put back ahead of each retry.  Returns the
    last sync()."""
    c = br.CASES[case]
    before = block.clone()
    rc = None
    for attempt in range(retries):
        if attempt:
            block.copy_(before)
        rd.render_backward_scene(scene, br.camera(gsr, case), c["W"], c["H"], grad_image_ptr=g_dev[0],
                                 grad_alpha_ptr=g_dev[1], scratch_ptr=scratch, **out_ptrs(block),
                                 k=c.get("k", 3.0), time=c.get("time"))
        rc = rd.sync()
        if rc == 0:
            break
    return rc


def device_g(torch, r):
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()  # noqa: E731
    return up(r["g_image"]), up(r["g_alpha"])


def check_fused_with_scratch(gsr, torch, rd, soa, scene, case, r, scratch, block):
    """The scratch's ten planes are the frame's record gradients (test_gpu_backward's check), and
    the scene gradients are bit-identical to a stand-alone project_backward fed that scratch."""
    from test_gpu_backward import assert_matches as assert_record_matches
    assert_record_matches(scratch.cpu().numpy(), [r], label=f"fused {case}: scratch")
    alone = new_block(torch, *block.shape)
    project(gsr, torch, gsr.Renderer(), scene, case, scratch, alone, cases=br.CASES, camera=br.camera)
    assert same_bits(block.cpu().numpy(), alone.cpu().numpy())
    assert alone.any()


@pytest.mark.parametrize("case", ["dense", "sparse_a", "4d", "faint"])
def test_fused_call_with_scratch_and_without(gpu, torch, bref, bscene_of, case):
    c = br.CASES[case]
    r = bref(case)
    soa, scene = bscene_of(c["scene"])
    narrays, n = soa.shape
    g_dev = device_g(torch, r)
    rd = gpu.Renderer()
    scratch = torch.full((10, n), 3.0, dtype=torch.float32, device="cuda")      # the call zeroes it
    block = new_block(torch, narrays, n)
    assert fused(gpu, torch, rd, scene, case, g_dev, scratch, block) == 0
    check_fused_with_scratch(gpu, torch, rd, soa, scene, case, r, scratch, block)
    # 8. without a scratch: the same up to the last bits of the blend's atomics; the map is
    # linear in its upstream, so the difference is bounded through the scale of that upstream
    null = new_block(torch, narrays, n)
    assert fused(gpu, torch, gpu.Renderer(), scene, case, g_dev, None, null) == 0
    up = scratch.cpu().numpy()
    ev = pr.evaluate(soa, pr.camera_values(gpu, br.camera(gpu, case)), c["W"], c["H"], c.get("time", 0.0), upstream=up)
    A = pr.scale(ev["abs"], narrays)
    A[:, ev["ambiguous"]] = np.nan                    # decided on the device either way: not compared
    got, want = null.cpu().numpy().astype(np.float64), block.cpu().numpy().astype(np.float64)
    pos = A > 0
    print(case, "NULL scratch: worst difference / A", float((np.abs(got - want)[pos] / A[pos]).max()), "of", TOL)
    assert pos.sum() > 100 and (np.abs(got - want)[pos] <= TOL * A[pos]).all()
    assert same_bits(got[A == 0], want[A == 0])


def test_fused_overflow_adds_nothing(gpu, torch, bref, bscene_of):
    """_backward_ref's overflowing frame: the first fused call overflows the pair buffer, sync()
    reports it and the prefilled outputs keep their bits; the re-render is complete."""
    case = "overflow"
    c = br.CASES[case]
    r = bref(case)
    soa, scene = bscene_of(c["scene"])
    narrays, n = soa.shape
    rd = gpu.Renderer()
    rd.reserve(n, 1024)
    g_dev = device_g(torch, r)
    scratch = torch.full((10, n), 3.0, dtype=torch.float32, device="cuda")
    block = new_block(torch, narrays, n, fill=1.5)
    assert fused(gpu, torch, rd, scene, case, g_dev, scratch, block, retries=1) == -5
    host = block.cpu().numpy()
    assert same_bits(host, np.full_like(host, 1.5))
    block.zero_()
    assert fused(gpu, torch, rd, scene, case, g_dev, scratch, block, retries=1) == 0
    assert rd.pair_count() > 1_000_000
    check_fused_with_scratch(gpu, torch, rd, soa, scene, case, r, scratch, block)


# ---------------------------------------------------------------- 10. frame policy

def test_depth_split_controller_untouched(gpu, torch, bref, bscene_of):
    case = "sparse_a"
    c = br.CASES[case]
    r = bref(case)
    soa, scene = bscene_of(c["scene"])
    cam = br.camera(gpu, case)
    rd = gpu.Renderer()
    rd.set_tuning(KNOB_SPLIT, 1)
    rd.set_tuning(KNOB_PM, 150)
    for _ in range(2):
        plain(gpu, torch, scene, cam, c["W"], c["H"], rd)
    before = (rd.get_tuning(KNOB_PM), rd.get_tuning(KNOB_STATE))
    scratch = torch.empty((10, soa.shape[1]), dtype=torch.float32, device="cuda")
    block = new_block(torch, *soa.shape)
    assert fused(gpu, torch, rd, scene, case, device_g(torch, r), scratch, block) == 0
    assert (rd.get_tuning(KNOB_PM), rd.get_tuning(KNOB_STATE)) == before
    check_fused_with_scratch(gpu, torch, rd, soa, scene, case, r, scratch, block)


def test_next_plain_frame_is_unaffected(gpu, torch, bref, bscene_of):
    """render, fused backward, render against render, render: the last frames are bit-identical."""
    case = "sparse_a"
    c = br.CASES[case]
    r = bref(case)
    soa, scene = bscene_of(c["scene"])
    cam_a, cam_b = br.camera(gpu, "sparse_a"), br.camera(gpu, "sparse_b")
    ra, rb = gpu.Renderer(), gpu.Renderer()
    for rd in (ra, rb):
        plain(gpu, torch, scene, cam_a, c["W"], c["H"], rd)
    block = new_block(torch, *soa.shape)
    assert fused(gpu, torch, ra, scene, case, device_g(torch, r), None, block) == 0
    assert block.any()
    last = [plain(gpu, torch, scene, cam_b, c["W"], c["H"], rd) for rd in (ra, rb)]
    assert same_bits(last[0], last[1]) and last[0].any()
