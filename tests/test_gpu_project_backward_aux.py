"""gsr_project_backward_aux and gsr_render_backward_scene_aux (Renderer.project_backward_aux,
Renderer.render_backward_scene_aux): the depth gradient d_z = dL/d(-Z) carried on to the scene
arrays, against the float64 torch.autograd reference of tests/_project_aux_ref.py
(tests/test_project_aux_ref.py pins it), and the fused call over eleven record planes.

Error measure and prefill rules are tests/test_gpu_project_backward.py's."""
import numpy as np
import pytest

import _backward_aux_ref as bar
import _backward_ref as br
import _project_aux_ref as par
import _project_ref as pr
from test_gpu_project_backward import new_block, out_ptrs, same_bits

pytestmark = pytest.mark.gpu

# E32_AUX: the largest error / A of the SAME eleven-component reference evaluated in float32
# torch, over every run of _project_aux_ref.RUNS (measured 6.04e-5, sparse_in "mixed", at a
# Gaussian close in front of the camera; tests/test_project_aux_ref.py asserts the constant against
# the measurement).  The GPU tolerance is 8 E32_AUX, that file's rule: another
# operation order and the device's division and sqrt.
E32_AUX = 6.5e-5
TOL = 8 * E32_AUX


@pytest.fixture(scope="module")
def torch(gpu):
    import torch as t
    assert t.cuda.is_available()
    return t


@pytest.fixture(scope="module")
def ref(gpu, tmp_path_factory):
    return lambda case, mode: par.reference(gpu, tmp_path_factory, case, mode)


@pytest.fixture(scope="module")
def scene_of(gpu, tmp_path_factory):
    cache = {}

    def get(case):
        if case not in cache:
            cache[case] = gpu.Scene.from_soa(pr.case_soa(gpu, tmp_path_factory, case))
        return cache[case]
    return get


def in_ptrs(up, which=par.INPUTS):
    return {"d_" + name + "_ptr": up[par.REC_ROWS[name]].data_ptr() if name in which else None for name in par.INPUTS}


def project_aux(gsr, torch, rd, scene, case, up, block, which=par.INPUTS, cases=pr.CASES, camera=pr.camera):
    c = cases[case]
    rd.project_backward_aux(scene, camera(gsr, case), c["W"], c["H"], **in_ptrs(up, which), **out_ptrs(block),
                            k=c.get("k", 3.0), time=c.get("time"))
    torch.cuda.synchronize()


def assert_matches(host, r, prefill=0.0, label=""):
    """The (narrays, n) host block against the reference: within TOL A where A > 0, bit-identical
    to the prefill where A = 0."""
    compared = 0
    for name, rows in pr.groups(host.shape[0]).items():
        got, want, A = host[rows], r["grad"][rows], r["A"][rows]
        pos = A > 0
        compared += int(pos.sum())
        assert np.isfinite(got).all()
        err = np.abs(got.astype(np.float64) - prefill - want)[pos] / A[pos]
        print(label, name, "worst error / A", float(err.max(initial=0.0)), "of", TOL)
        assert same_bits(got[~pos], np.full_like(got[~pos], prefill)), (label, name, "A = 0 entries changed")
        bad = np.argwhere((np.abs(got.astype(np.float64) - prefill - want) > TOL * A) & pos)
        assert len(bad) == 0, (label, name, bad[:8], float(err.max()))
    assert compared > 0, (label, "nothing to compare")


# ---------------------------------------------------------------- 1. against autograd

@pytest.mark.parametrize("case,mode", par.RUNS)
def test_matches_reference(gpu, torch, ref, scene_of, case, mode):
    r = ref(case, mode)
    narrays, n = r["soa"].shape
    up = torch.from_numpy(np.array(r["upstream"])).cuda()
    rd = gpu.Renderer()
    block = new_block(torch, narrays, n)
    project_aux(gpu, torch, rd, scene_of(case), case, up, block)
    host = block.cpu().numpy()
    assert_matches(host, r, label=f"{case} {mode}")
    if mode == "z":
        # the depth reaches the position and nothing else ...
        live = r["valid"] & r["upstream"].any(0)
        assert live.sum() > 50 and host[0:3, live].any(0).all()
        assert not host[3:38].any()
        if narrays == 49:   # ... but, through the position, trbf_center and the motion arrays
            assert not host[39].any()
            moving = live & (np.abs(pr.CASES[case]["time"] - r["soa"][38]) > 1e-3)
            assert moving.sum() > 50 and (host[38, live] != 0).mean() > 0.9 and host[40:49, moving].any(0).all()
    # a prefilled block keeps its bits where A = 0 and at every skipped Gaussian
    block = new_block(torch, narrays, n, fill=1.5)
    project_aux(gpu, torch, rd, scene_of(case), case, up, block)
    filled = block.cpu().numpy()
    skipped = ~r["valid"] | ~r["upstream"].any(0)
    keep = (r["A"] == 0) | skipped[None]
    assert same_bits(filled[keep], np.full_like(filled[keep], 1.5))
    assert (filled[:, ~skipped] != 1.5).any(axis=0).all()


# ---------------------------------------------------------------- 2. determinism

@pytest.mark.parametrize("case", ["sparse_in", "4d"])
def test_two_calls_give_identical_bits(gpu, torch, ref, scene_of, case):
    r = ref(case, "mixed")
    narrays, n = r["soa"].shape
    up = torch.from_numpy(np.array(r["upstream"])).cuda()
    hosts = []
    for _ in range(2):
        block = new_block(torch, narrays, n)
        project_aux(gpu, torch, gpu.Renderer(), scene_of(case), case, up, block)
        hosts.append(block.cpu().numpy())
    assert same_bits(hosts[0], hosts[1]) and hosts[0].any()


# ---------------------------------------------------------------- 3. skipped Gaussians

def test_skipped_gaussians_keep_their_value(gpu, torch, ref, scene_of):
    """A Gaussian whose eleven upstream entries are all +-0 keeps its prefill; so does a culled
    one whatever its d_z; one whose d_z alone is non-zero takes part."""
    case = "sparse_in"
    r = ref(case, "mixed")
    narrays, n = r["soa"].shape
    upstream = np.array(r["upstream"])
    pick = np.random.default_rng(5).random(n)
    zeroed, z_alone = pick < 1 / 3, (pick >= 1 / 3) & (pick < 2 / 3)
    upstream[:, zeroed] = 0.0
    upstream[::2, zeroed] = -0.0
    upstream[:10, z_alone] = 0.0
    invalid_live = ~r["valid"] & (upstream[10] != 0)
    valid_zero = r["valid"] & ~upstream.any(0)
    valid_z = r["valid"] & z_alone & (upstream[10] != 0)
    print("culled with d_z", int(invalid_live.sum()), "valid, all zero", int(valid_zero.sum()), "valid, d_z alone",
          int(valid_z.sum()))
    assert invalid_live.sum() >= 100 and valid_zero.sum() >= 100 and valid_z.sum() >= 100
    block = new_block(torch, narrays, n, fill=1.5)
    project_aux(gpu, torch, gpu.Renderer(), scene_of(case), case, torch.from_numpy(upstream).cuda(), block)
    host = block.cpu().numpy()
    assert same_bits(host[:, invalid_live], np.full_like(host[:, invalid_live], 1.5))
    assert same_bits(host[:, valid_zero], np.full_like(host[:, valid_zero], 1.5))
    assert (host[0:3, valid_z] != 1.5).any(axis=0).all()


# ---------------------------------------------------------------- 4. without d_z: gsr_project_backward

@pytest.mark.parametrize("case", ["rot", "sh3", "4d"])
def test_without_dz_is_project_backward(gpu, torch, ref, scene_of, case):
    """The old entry point with the old struct and the new one with d_z = NULL: identical bytes."""
    from test_gpu_project_backward import project
    r = ref(case, "mixed")
    narrays, n = r["soa"].shape
    up = torch.from_numpy(np.array(r["upstream"])).cuda()
    rd = gpu.Renderer()
    old, new = new_block(torch, narrays, n), new_block(torch, narrays, n)
    project(gpu, torch, rd, scene_of(case), case, up, old)
    project_aux(gpu, torch, rd, scene_of(case), case, up, new, which=("color", "opacity", "conic", "center"))
    assert same_bits(old.cpu().numpy(), new.cpu().numpy()) and old.any()


# ---------------------------------------------------------------- 5. the fused call

def fused(gsr, torch, rd, scene, case, kw_in, feat_grad, scratch, block):
    """One complete fused frame of _backward_ref's `case` into block and feat_grad
    (accumulating): up to three renders until sync() == 0."""
    c = br.CASES[case]
    before = block.clone(), None if feat_grad is None else feat_grad.clone()
    for attempt in range(3):
        if attempt:
            block.copy_(before[0])
            if feat_grad is not None:
                feat_grad.copy_(before[1])
        rd.render_backward_scene_aux(scene, br.camera(gsr, case), c["W"], c["H"], **kw_in, feat_grad_ptr=feat_grad,
                                     scratch_ptr=scratch, **out_ptrs(block), k=c.get("k", 3.0), time=c.get("time"))
        if rd.sync() == 0:
            return
    raise AssertionError("fused frame still incomplete after three renders")


@pytest.mark.parametrize("case,sp", [("dense", bar.ALL4), ("4d", bar.spec(29, alpha=False))])
def test_fused_call_equals_the_two_call_chain(gpu, torch, orc, tmp_path_factory, case, sp):
    """With a caller's scratch: its eleven planes and the feature gradients are the frame's record
    gradients (test_gpu_backward_aux's check), and the projection run alone on the scratch the
    fused call left gives the fused call's own outputs bit for bit."""
    from test_gpu_backward_aux import assert_matches as assert_record_matches, device_in
    c = br.CASES[case]
    r = bar.reference(gpu, orc, tmp_path_factory, case, sp)
    soa = br.scenes(gpu, orc, tmp_path_factory)[c["scene"]]
    scene = gpu.Scene.from_soa(soa)
    narrays, n = soa.shape
    nfeat = r["nfeat"]
    rd = gpu.Renderer()
    scratch = torch.full((11, n), 3.0, dtype=torch.float32, device="cuda")      # the call zeroes it
    feat_grad = torch.zeros((nfeat, n), dtype=torch.float32, device="cuda") if nfeat else None
    block = new_block(torch, narrays, n)
    fused(gpu, torch, rd, scene, case, device_in(torch, r), feat_grad, scratch, block)
    planes = scratch.cpu().numpy()
    if nfeat:
        planes = np.concatenate([planes, feat_grad.cpu().numpy()])
    assert_record_matches(planes, [r], nfeat, label=f"fused {case}: scratch")
    assert planes[10].any()
    alone = new_block(torch, narrays, n)
    project_aux(gpu, torch, gpu.Renderer(), scene, case, scratch, alone, cases=br.CASES, camera=br.camera)
    assert same_bits(block.cpu().numpy(), alone.cpu().numpy()) and alone.any()
    if narrays == 49:
        assert alone[38].any() and alone[40:49].any()
    # and the depth gradient is in there: without the z plane the positions differ
    without = new_block(torch, narrays, n)
    project_aux(gpu, torch, gpu.Renderer(), scene, case, scratch, without,
                which=("color", "opacity", "conic", "center"), cases=br.CASES, camera=br.camera)
    assert not same_bits(without[0:3].cpu().numpy(), alone[0:3].cpu().numpy())
    # without a caller's scratch (the context's workspace, grown to 11 n floats): the same up to
    # the last bits of the blend's atomics; the projection is linear in its upstream, so the
    # difference is bounded through the scale of that upstream (test_gpu_project_backward's rule)
    null = new_block(torch, narrays, n)
    null_feat = torch.zeros((nfeat, n), dtype=torch.float32, device="cuda") if nfeat else None
    fused(gpu, torch, gpu.Renderer(), scene, case, device_in(torch, r), null_feat, None, null)
    ev = par.evaluate(soa, pr.camera_values(gpu, br.camera(gpu, case)), c["W"], c["H"], c.get("time", 0.0),
                      upstream=scratch.cpu().numpy())
    A = pr.scale(ev["abs"], narrays)
    A[:, ev["ambiguous"]] = np.nan                    # decided on the device either way: not compared
    got, want = null.cpu().numpy().astype(np.float64), block.cpu().numpy().astype(np.float64)
    pos = A > 0
    print(case, "NULL scratch: worst difference / A", float((np.abs(got - want)[pos] / A[pos]).max()), "of", TOL)
    assert pos.sum() > 100 and (np.abs(got - want)[pos] <= TOL * A[pos]).all()
    assert same_bits(got[A == 0], want[A == 0])
    if nfeat:
        assert_record_matches(np.concatenate([planes[:11], null_feat.cpu().numpy()]), [r], nfeat,
                              label=f"fused {case}: feature gradients, no scratch")


def test_fused_first_ten_planes_where_they_were(gpu, torch, orc, tmp_path_factory):
    """Image and alpha upstream only: planes 0..9 of the eleven-plane scratch are
    gsr_render_backward_scene's (tests/test_gpu_backward.py's check at its offsets; the centre
    planes gsr_densify_accumulate reads are 8 and 9), plane 10 stays zero, and without a scratch
    (the context's workspace) the outputs are gsr_render_backward_scene's within the tolerance."""
    from test_gpu_backward import assert_matches as assert_base, device_g
    case, g = "dense", (5, False, True, True)
    c = br.CASES[case]
    r = br.reference(gpu, orc, tmp_path_factory, case, g)
    soa = br.scenes(gpu, orc, tmp_path_factory)[c["scene"]]
    scene = gpu.Scene.from_soa(soa)
    narrays, n = soa.shape
    g_dev = device_g(torch, r)
    kw_in = dict(grad_image_ptr=g_dev[0], grad_alpha_ptr=g_dev[1])
    rd = gpu.Renderer()
    scratch = torch.full((11, n), 3.0, dtype=torch.float32, device="cuda")
    block = new_block(torch, narrays, n)
    fused(gpu, torch, rd, scene, case, kw_in, None, scratch, block)
    host = scratch.cpu().numpy()
    assert_base(host[:10], [r], label="fused aux, no aux inputs")
    assert not host[10].any()
    old_scratch = torch.full((10, n), 3.0, dtype=torch.float32, device="cuda")
    old = new_block(torch, narrays, n)
    rd.render_backward_scene(scene, br.camera(gpu, case), c["W"], c["H"], grad_image_ptr=g_dev[0],
                             grad_alpha_ptr=g_dev[1], scratch_ptr=old_scratch, **out_ptrs(old))
    assert rd.sync() == 0
    assert_base(old_scratch.cpu().numpy(), [r], label="gsr_render_backward_scene")
    # without a scratch: the plain fused call's outputs up to the last bits of the atomics
    null = new_block(torch, narrays, n)
    fused(gpu, torch, gpu.Renderer(), scene, case, kw_in, None, None, null)
    ev = par.evaluate(soa, pr.camera_values(gpu, br.camera(gpu, case)), c["W"], c["H"], upstream=host)
    A = pr.scale(ev["abs"], narrays)
    A[:, ev["ambiguous"]] = np.nan
    got, want = null.cpu().numpy().astype(np.float64), old.cpu().numpy().astype(np.float64)
    pos = A > 0
    assert pos.sum() > 100 and (np.abs(got - want)[pos] <= TOL * A[pos]).all()
    assert same_bits(got[A == 0], want[A == 0])
