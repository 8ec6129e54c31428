"""gsr_render_backward_aux (Renderer.render_backward_aux): the per-Gaussian gradients of the
blend with its depth and feature planes against the float64 reference of
tests/_backward_aux_ref.py, which tests/test_backward_aux_ref.py pins to the unmodified oracle
and to its own finite differences.

Error measure, as tests/test_gpu_backward.py: |got - reference| / A per component and Gaussian,
A the reference's scale plane.  Where A = 0 the output keeps its prefilled value bit for bit.
The upstream gradients are zeroed at the reference's ambiguous pixels on both sides.  All
outputs live in ONE (11 + nfeat, n) block (colour 3, opacity 1, conic 4, centre 2, z 1, the
features), so a write outside a plane lands in a checked one."""
import numpy as np
import pytest

import _backward_aux_ref as bar
import _backward_ref as br
from test_gpu_backward import KNOB_BLEND_EXP, KNOB_PM, KNOB_SPLIT, KNOB_STATE, plain, same_bits, tiling_of

pytestmark = pytest.mark.gpu

# E32_AUX: the largest error / A of the SAME reference evaluated in float32 numpy, over every
# run of _backward_aux_ref.RUNS_AUX and every kind of output (measured 5.47e-6;
# tests/test_backward_aux_ref.py asserts the constant against the measurement).  The GPU
# tolerance is 8 E32_AUX, the factor of tests/test_gpu_backward.py for the same reasons: a
# different exp, FMA contraction and the arbitrary order of the atomics.  It is measured against
# the reference, never against the kernel.
E32_AUX = 5.5e-6
TOL_AUX = 8 * E32_AUX

BASE = ("color", "opacity", "conic", "center")


@pytest.fixture(scope="module")
def torch(gpu):
    import torch as t
    assert t.cuda.is_available()
    return t


@pytest.fixture(scope="module")
def ref(gpu, orc, tmp_path_factory):
    return lambda case, sp=bar.ALL4: bar.reference(gpu, orc, tmp_path_factory, case, sp)


@pytest.fixture(scope="module")
def scene_of(gpu, orc, tmp_path_factory):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = gpu.Scene.from_soa(br.scenes(gpu, orc, tmp_path_factory)[name])
        return cache[name]
    return get


def dev(torch, a):
    # (a copy: the references are read-only)
    return None if a is None else torch.from_numpy(np.array(a, np.float32)).cuda()


def device_in(torch, r, drop=()):
    """The reference's upstream gradients (already zero at ambiguous pixels) and feature values
    on the device: keywords of render_backward_aux.  drop: upstream names passed as None."""
    g = dict(zip(("image", "alpha", "depth", "feat"), bar.upstream_of(r)))
    kw = {f"grad_{k}_ptr": dev(torch, None if k in drop else v) for k, v in g.items()}
    kw["features_ptr"], kw["nfeat"] = dev(torch, r["features"]), r["nfeat"]
    return kw


def new_block(torch, n, nfeat, fill=0.0):
    return torch.full((11 + nfeat, n), fill, dtype=torch.float32, device="cuda")


OUT_KW = {"color": "color_ptr", "opacity": "opacity_ptr", "conic": "conic_ptr", "center": "center_ptr", "z": "z_ptr",
          "feat": "feat_grad_ptr"}


def out_kw(block, nfeat, what):
    rows = bar.rows(nfeat)
    return {OUT_KW[k]: block[rows[k]].data_ptr() for k in what if k in rows}


def backward_into(gsr, rd, scene, case, kw_in, block, nfeat, what=None):
    """One complete frame of `case` into the planes `what` of block (accumulating): up to three
    renders until sync() == 0, the block put back ahead of each retry."""
    c = br.CASES[case]
    what = [k for k, _ in bar.kinds(nfeat)] if what is None else what
    before = block.clone()
    for attempt in range(3):
        if attempt:
            block.copy_(before)
        rd.render_backward_aux(scene, br.camera(gsr, case), c["W"], c["H"], **kw_in, **out_kw(block, nfeat, what),
                               k=c.get("k", 3.0), tiling=tiling_of(gsr, case), time=c.get("time"))
        if rd.sync() == 0:
            return
    raise AssertionError("backward frame still incomplete after three renders")


def assert_matches(block, refs, nfeat, what=None, prefill=0.0, label="", tol=TOL_AUX):
    """Planes `what` of the (11 + nfeat, n) host block against the sum of the references `refs`
    (scales add); every other plane, and every entry with A = 0, keeps the prefill bit for bit."""
    rows = bar.rows(nfeat)
    what = list(rows) if what is None else what
    worst = 0.0
    for kind in rows:
        got = block[rows[kind]]
        if kind not in what:
            assert same_bits(got, np.full_like(got, prefill)), (label, kind, "not asked for, yet written")
            continue
        want = sum(r[kind].astype(np.float64) for r in refs)
        A = sum(r["A_" + kind] for r in refs)
        pos = A > 0
        err = np.abs(got.astype(np.float64) - prefill - want)[pos] / A[pos]
        print(label, kind, "worst error / A", float(err.max(initial=0.0)), "of", tol)
        worst = max(worst, float(err.max(initial=0.0)))
        assert np.isfinite(got).all()
        assert same_bits(got[~pos], np.full_like(got[~pos], prefill)), (label, kind, "A = 0 entries changed")
        bad = np.argwhere((np.abs(got.astype(np.float64) - prefill - want) > tol * A) & pos)
        assert len(bad) == 0, (label, kind, bad[:8], float(err.max()))
    assert worst > 0, (label, "nothing to compare")
    return worst


# ---------------------------------------------------------------- 1. all outputs, every run

@pytest.mark.parametrize("case,sp", [(c, s) for c, s in bar.RUNS_AUX if c != "overflow"])
def test_all_outputs_match_reference(gpu, torch, ref, scene_of, case, sp):
    r = ref(case, sp)
    assert r["takes"].sum() > 500 and br.mask_share(r) <= bar.MASK_SHARE_CAP
    if case == "faint":
        assert r["takes"].max() > 300 and len(r["rec"]["order"]) == 3000
    nfeat = r["nfeat"]
    block = new_block(torch, r["rec"]["n"], nfeat)
    backward_into(gpu, gpu.Renderer(), scene_of(br.CASES[case]["scene"]), case, device_in(torch, r), block, nfeat)
    # (an output whose upstream is not given has A = 0 in the reference too: it keeps the prefill)
    assert_matches(block.cpu().numpy(), [r], nfeat, label=f"{case} {sp}")


# ---------------------------------------------------------------- 2. subsets of outputs and upstreams

def test_output_subsets(gpu, torch, ref, scene_of):
    """Each output alone, all together, z + feat only (the one-sweep kernel), colour + z + feat:
    planes not asked for keep a -7.25 prefill."""
    r = ref("dense", bar.ALL4)
    nfeat, n = r["nfeat"], r["rec"]["n"]
    kw_in = device_in(torch, r)
    rd = gpu.Renderer()
    names = [k for k, _ in bar.kinds(nfeat)]
    rows = bar.rows(nfeat)
    for what in [(k,) for k in names] + [tuple(names), ("z", "feat"), ("color", "z", "feat"), ("opacity", "feat")]:
        block = new_block(torch, n, nfeat, fill=-7.25)
        for k in what:
            block[rows[k]] = 0.0
        backward_into(gpu, rd, scene_of("dense"), "dense", kw_in, block, nfeat, what)
        host = block.cpu().numpy()
        for k in names:
            if k not in what:
                assert same_bits(host[rows[k]], np.full_like(host[rows[k]], -7.25)), (what, k)
                host[rows[k]] = 0.0
        assert_matches(host, [r], nfeat, what, label=str(what))


@pytest.mark.parametrize("given", [("image", "depth"), ("alpha", "feat"), ("depth",), ("feat",), ("image", "alpha")])
def test_upstream_subsets(gpu, torch, orc, tmp_path_factory, scene_of, given):
    """A subset of the upstream gradients NULL, every output asked for: the reference of that
    subset; the outputs whose upstream is missing keep a -7.25 prefill."""
    sp = bar.spec(21, image="image" in given, alpha="alpha" in given, depth="depth" in given, nfeat=4,
                  feat_up="feat" in given)
    r = bar.reference(gpu, orc, tmp_path_factory, "dense", sp)
    nfeat, n = 4, r["rec"]["n"]
    rows = bar.rows(nfeat)
    block = new_block(torch, n, nfeat, fill=-7.25)
    untouched = [k for k, up in (("color", "image"), ("z", "depth"), ("feat", "feat")) if up not in given]
    for k in rows:
        if k not in untouched:
            block[rows[k]] = 0.0
    backward_into(gpu, gpu.Renderer(), scene_of("dense"), "dense", device_in(torch, r), block, nfeat)
    host = block.cpu().numpy()
    for k in untouched:
        assert same_bits(host[rows[k]], np.full_like(host[rows[k]], -7.25)), (given, k)
        assert not r["A_" + k].any()
        host[rows[k]] = 0.0
    assert_matches(host, [r], nfeat, label=str(given))


def test_eight_feature_subsets(gpu, torch, orc, tmp_path_factory, ref, scene_of):
    """The packed path's other instantiations: 8 features with the geometry and no depth gradient;
    depth + 8 features with only the linear outputs (one sweep, no gathers); and the latter with
    no depth gradient either."""
    rd = gpu.Renderer()
    r = bar.reference(gpu, orc, tmp_path_factory, "dense", bar.spec(24, depth=False, nfeat=8))
    n, rows = r["rec"]["n"], bar.rows(8)
    block = new_block(torch, n, 8, fill=-7.25)
    for k in rows:
        if k != "z":
            block[rows[k]] = 0.0
    backward_into(gpu, rd, scene_of("dense"), "dense", device_in(torch, r), block, 8)
    host = block.cpu().numpy()
    assert same_bits(host[rows["z"]], np.full_like(host[rows["z"]], -7.25)) and not r["A_z"].any()
    host[rows["z"]] = 0.0
    assert_matches(host, [r], 8, label="8 features, no depth gradient")
    linear = ("color", "z", "feat")
    block = new_block(torch, n, 8)
    backward_into(gpu, rd, scene_of("dense"), "dense", device_in(torch, r), block, 8, ("color", "feat"))
    assert_matches(block.cpu().numpy(), [r], 8, ("color", "feat"), label="8 features, linear outputs only")
    r = ref("dense", bar.spec(24, nfeat=8))
    block = new_block(torch, n, 8)
    backward_into(gpu, rd, scene_of("dense"), "dense", device_in(torch, r), block, 8, linear)
    assert_matches(block.cpu().numpy(), [r], 8, linear, label="depth + 8 features, linear outputs only")


# ---------------------------------------------------------------- 3. untouched outputs and Gaussians

def test_z_untouched_without_depth_gradient(gpu, torch, ref, scene_of):
    """The same run with d_grad_depth withheld: d_z keeps its bytes, whatever they are."""
    r = ref("dense", bar.ALL4)
    nfeat, n = r["nfeat"], r["rec"]["n"]
    rows = bar.rows(nfeat)
    block = new_block(torch, n, nfeat)
    noise = np.random.default_rng(3).standard_normal(n).astype(np.float32)
    block[rows["z"]] = torch.from_numpy(noise).cuda()
    backward_into(gpu, gpu.Renderer(), scene_of("dense"), "dense", device_in(torch, r, drop=("depth",)), block, nfeat)
    host = block.cpu().numpy()
    assert same_bits(host[rows["z"]][0], noise)
    assert host[rows["feat"]].any() and host[rows["color"]].any()


@pytest.mark.parametrize("case,sp", [("dense99", bar.spec(26, nfeat=3)), ("sparse_a", bar.ALL8)])
def test_uncomposited_gaussians_keep_their_value(gpu, torch, ref, scene_of, case, sp):
    """Gaussians no pixel composited (render_contrib's count of the same frame is 0) keep a
    prefilled 1.5 in every plane, z and the features included."""
    c = br.CASES[case]
    r = ref(case, sp)
    nfeat, n = r["nfeat"], r["rec"]["n"]
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
    block = new_block(torch, n, nfeat, fill=1.5)
    backward_into(gpu, rd, scene, case, device_in(torch, r), block, nfeat)
    host = block.cpu().numpy()
    assert same_bits(host[:, idle], np.full_like(host[:, idle], 1.5))
    assert (host[10:, ~idle] != 1.5).any(axis=0).mean() > 0.9    # and the others' z / features moved


# ---------------------------------------------------------------- 4. no aux inputs: gsr_render_backward

@pytest.mark.parametrize("case,g", [("dense", (5, False, True, True)), ("sparse_a", (8, False, True, True))])
def test_no_aux_inputs_is_render_backward(gpu, torch, orc, tmp_path_factory, scene_of, case, g):
    """Without d_grad_depth, features, d_z and d_feat the aux entry point and gsr_render_backward
    both meet tests/_backward_ref.py's reference within tests/test_gpu_backward.py's TOL."""
    from test_gpu_backward import assert_matches as assert_base, backward_into as base_into, device_g
    c = br.CASES[case]
    r = br.reference(gpu, orc, tmp_path_factory, case, g)
    n = r["rec"]["n"]
    g_dev = device_g(torch, r)
    rd = gpu.Renderer()
    old = torch.zeros((10, n), dtype=torch.float32, device="cuda")
    base_into(gpu, rd, scene_of(c["scene"]), case, g_dev, old)
    assert_base(old.cpu().numpy(), [r], label="gsr_render_backward")
    new = new_block(torch, n, 0)
    kw_in = dict(grad_image_ptr=g_dev[0], grad_alpha_ptr=g_dev[1])
    backward_into(gpu, rd, scene_of(c["scene"]), case, kw_in, new, 0, BASE)
    host = new.cpu().numpy()
    assert not host[10].any()
    assert_base(host[:10], [r], label="gsr_render_backward_aux, no aux inputs")


# ---------------------------------------------------------------- 5. linearity against the forward kernel

def render_aux_planes(gsr, torch, rd, scene, case, feats):
    """depth (H, W) and feature planes (nfeat, H, W) of gsr_render_aux, float64 on the host."""
    c = br.CASES[case]
    nfeat = feats.shape[0]
    depth = torch.full((c["H"], c["W"]), float("nan"), dtype=torch.float32, device="cuda")
    planes = torch.full((nfeat, c["H"], c["W"]), float("nan"), dtype=torch.float32, device="cuda")
    f_dev = dev(torch, feats)
    for _ in range(3):
        rd.render_aux(scene, br.camera(gsr, case), c["W"], c["H"], depth_ptr=depth.data_ptr(),
                      features_ptr=f_dev.data_ptr(), nfeat=nfeat, feat_out_ptr=planes.data_ptr(), k=c.get("k", 3.0))
        if rd.sync() == 0:
            return depth.cpu().numpy().astype(np.float64), planes.cpu().numpy().astype(np.float64)
    raise AssertionError("aux frame still incomplete after three renders")


@pytest.mark.parametrize("case", ["dense", "sparse_a"])
def test_linearity_against_render_aux(gpu, torch, ref, scene_of, case):
    """depth = sum_i z_i (alpha T)_i per pixel, so with g_D = 1 everywhere sum_i z_i d_z[i] is
    the sum of gsr_render_aux's depth plane, the oracle-checked forward; and per feature with
    g_f = 1.  Bounds: TOL_AUX sum_i |z_i| A_z[i] for the backward (A_z with g = 1 is d_z's own
    exact value, taken from the reference's weights) plus 2^-20 sum |plane| for the forward's
    accumulation (tests/test_gpu_aux.py).  No pixel is masked here: an ambiguous decision falls
    the same way in both kernels, which share the step."""
    c = br.CASES[case]
    r = ref(case, bar.ALL8)
    n, nfeat, feats = r["rec"]["n"], 8, r["features"]
    scene = scene_of(c["scene"])
    rd = gpu.Renderer()
    depth, planes = render_aux_planes(gpu, torch, rd, scene, case, feats)
    ones = torch.ones((nfeat, c["H"], c["W"]), dtype=torch.float32, device="cuda")
    z = r["rec"]["z"][0]
    # sum over pixels of alpha T per Gaussian, float64: the reference's colour weights with g = 1
    w_ref = bar.evaluate(r["rec"], c["W"], c["H"], g_depth=np.ones((c["H"], c["W"])), tiling=c.get("tiling"),
                         zero_masked=False)
    wsum = w_ref["A_z"][0]
    assert (wsum > 0).sum() > 50
    # g_D = 1 only
    block = new_block(torch, n, 0)
    backward_into(gpu, rd, scene, case, dict(grad_depth_ptr=ones[0]), block, 0, ("z",))
    dz = block.cpu().numpy()[10].astype(np.float64)
    lhs, rhs = float((z * dz).sum()), float(depth.sum())
    bound = TOL_AUX * float((np.abs(z) * wsum).sum()) + 2.0 ** -20 * float(np.abs(depth).sum())
    print(case, "depth: sum z dz", lhs, "sum depth", rhs, "difference", abs(lhs - rhs), "bound", bound)
    assert rhs > 100 and abs(lhs - rhs) <= bound
    # g_f = 1 only, eight features
    block = new_block(torch, n, nfeat)
    kw_in = dict(grad_feat_ptr=ones, features_ptr=dev(torch, feats), nfeat=nfeat)
    backward_into(gpu, rd, scene, case, kw_in, block, nfeat, ("feat",))
    df = block.cpu().numpy()[11:].astype(np.float64)
    for f in range(nfeat):
        lhs, rhs = float((feats[f].astype(np.float64) * df[f]).sum()), float(planes[f].sum())
        bound = TOL_AUX * float((np.abs(feats[f]) * wsum).sum()) + 2.0 ** -20 * float(np.abs(planes[f]).sum())
        print(case, "feature", f, "difference", abs(lhs - rhs), "bound", bound)
        assert abs(lhs - rhs) <= bound
    assert np.abs(planes).sum() > 100


# ---------------------------------------------------------------- 6. frame behaviour

def test_two_cameras_accumulate(gpu, torch, ref, scene_of):
    ra, rb = ref("sparse_a", bar.ALL8), ref("sparse_b", bar.spec(28, nfeat=8))
    block = new_block(torch, ra["rec"]["n"], 8)
    rd = gpu.Renderer()
    backward_into(gpu, rd, scene_of("sparse"), "sparse_a", device_in(torch, ra), block, 8)
    backward_into(gpu, rd, scene_of("sparse"), "sparse_b", device_in(torch, rb), block, 8)
    only_a = (ra["A_z"][0] > 0) & ~(rb["A_z"][0] > 0)
    assert only_a.sum() > 50 and ((rb["A_z"][0] > 0) & ~(ra["A_z"][0] > 0)).sum() > 50
    assert_matches(block.cpu().numpy(), [ra, rb], 8, label="two cameras")


def test_overflow_frame_adds_nothing(gpu, torch, ref, scene_of):
    """tests/test_gpu_backward.py's overflowing frame: the first render overflows the pair buffer
    and leaves the prefilled planes exactly as they were; the re-render is complete and matches
    the reference.  The upstream gradients are confined to the case's region."""
    case, sp = "overflow", bar.spec(32, nfeat=4)
    c = br.CASES[case]
    r = ref(case, sp)
    n, nfeat = r["rec"]["n"], 4
    compared = ~r["mask"] & (r["takes"] > 0)
    assert compared.sum() >= 80 and r["takes"].max() > 200
    rd = gpu.Renderer()
    rd.reserve(n, 1024)
    block = new_block(torch, n, nfeat, fill=1.5)
    kw = dict(device_in(torch, r), **out_kw(block, nfeat, list(bar.rows(nfeat))))
    rd.render_backward_aux(scene_of("overflow"), br.camera(gpu, case), c["W"], c["H"], **kw)
    assert rd.sync() == -5                      # overflow reported and buffer grown
    host = block.cpu().numpy()
    assert same_bits(host, np.full_like(host, 1.5))
    block.zero_()
    rd.render_backward_aux(scene_of("overflow"), br.camera(gpu, case), c["W"], c["H"], **kw)
    assert rd.sync() == 0
    assert rd.pair_count() > 1_000_000
    assert_matches(block.cpu().numpy(), [r], nfeat, label="overflow, re-rendered")


def test_depth_split_controller_untouched(gpu, torch, ref, scene_of):
    case = "sparse_a"
    c = br.CASES[case]
    r = ref(case, bar.ALL8)
    cam = br.camera(gpu, case)
    rd = gpu.Renderer()
    rd.set_tuning(KNOB_SPLIT, 1)
    rd.set_tuning(KNOB_PM, 150)
    for _ in range(2):
        plain(gpu, torch, scene_of("sparse"), cam, c["W"], c["H"], rd)
    before = (rd.get_tuning(KNOB_PM), rd.get_tuning(KNOB_STATE))
    block = new_block(torch, r["rec"]["n"], 8)
    backward_into(gpu, rd, scene_of("sparse"), case, device_in(torch, r), block, 8)
    assert (rd.get_tuning(KNOB_PM), rd.get_tuning(KNOB_STATE)) == before
    assert_matches(block.cpu().numpy(), [r], 8, label="split on")


@pytest.mark.parametrize("blend_exp", [0, 1])
def test_exact_blend_whatever_the_knob(gpu, torch, ref, scene_of, blend_exp):
    r = ref("dense", bar.ALL4)
    rd = gpu.Renderer()
    rd.set_tuning(KNOB_BLEND_EXP, blend_exp)
    block = new_block(torch, r["rec"]["n"], 4)
    backward_into(gpu, rd, scene_of("dense"), "dense", device_in(torch, r), block, 4)
    assert rd.get_tuning(KNOB_BLEND_EXP) == blend_exp
    assert_matches(block.cpu().numpy(), [r], 4, label=f"blend_exp {blend_exp}")


def test_next_plain_frame_is_unaffected(gpu, torch, ref, scene_of):
    """render, backward, render against render, render: the last frames are bit-identical."""
    case = "sparse_a"
    c = br.CASES[case]
    r = ref(case, bar.ALL8)
    cam_a, cam_b = br.camera(gpu, "sparse_a"), br.camera(gpu, "sparse_b")
    ra, rb = gpu.Renderer(), gpu.Renderer()
    for rd in (ra, rb):
        plain(gpu, torch, scene_of("sparse"), cam_a, c["W"], c["H"], rd)
    block = new_block(torch, r["rec"]["n"], 8)
    backward_into(gpu, ra, scene_of("sparse"), case, device_in(torch, r), block, 8)
    last = [plain(gpu, torch, scene_of("sparse"), cam_b, c["W"], c["H"], rd) for rd in (ra, rb)]
    assert same_bits(last[0], last[1]) and last[0].any()


def test_smaller_frame_after_a_larger_one(gpu, torch, orc, tmp_path_factory, scene_of):
    """One context: sparse_a (2000 Gaussians, 8 features: aux_z and aux_pack at their high-water
    mark), then dense with depth + 6 features on the same context matches its reference.  That
    the second frame regrows nothing is not observable through the interface and is not asserted:
    the workspaces grow by high-water mark (DevBuf::reserve), which this order exercises."""
    big = bar.reference(gpu, orc, tmp_path_factory, "sparse_a", bar.ALL8)
    sp = bar.spec(33, image=False, alpha=False, nfeat=6)
    small = bar.reference(gpu, orc, tmp_path_factory, "dense", sp)
    assert small["rec"]["n"] < big["rec"]["n"]
    rd = gpu.Renderer()
    block = new_block(torch, big["rec"]["n"], 8)
    backward_into(gpu, rd, scene_of("sparse"), "sparse_a", device_in(torch, big), block, 8)
    block = new_block(torch, small["rec"]["n"], 6)
    backward_into(gpu, rd, scene_of("dense"), "dense", device_in(torch, small), block, 6)
    assert_matches(block.cpu().numpy(), [small], 6, label="dense after sparse_a")
