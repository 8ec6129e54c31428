"""gsr_image_loss on the device (gaussianrenderer_amd.image_loss): the gradient and the four
loss values against the float64 reference (tests/_loss_ref.py) over every case and weighting,
within 8 x what single precision alone costs (E32, EL32: measured on the reference itself in
tests/test_loss_ref.py, never on the kernel); exact zeros for equal images; guard words around
every buffer the call writes; the value-only and gradient-only modes, grad_scale, two streams;
and a closed render -> loss -> backward -> step loop that descends."""
import numpy as np
import pytest

import _loss_ref as lr
from test_gpu_adam import DevPlanes, zeros_like_groups
from test_gpu_parity import CAMS, cam_for
from test_gpu_scene_ops import dense_soa, dev, exact_renderer, frame, same_bits
from test_loss_ref import E32, EL32

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
MARGIN = 8          # another operation order and the device's division
NAN_BITS = 0x7FC0BEEF


@pytest.fixture(scope="module")
def torch(gpu):
    import torch as t
    assert t.cuda.is_available()
    return t


def run(gsr, torch, x, y, weights=(0.8, 0.0, 0.2), grad=True, value=True, grad_scale=1.0, stream=0):
    """One call on fresh buffers, every one of them offset by a word (addresses 4 mod 16) and
    fenced by sentinel words, the scratch at exactly the queried size and full of NaNs:
    (gradient (3, H, W) or None, the four values or None).  Checks the sentinels and that the
    inputs kept their bits."""
    _, H, W = x.shape
    nbytes = gsr.image_loss_scratch_bytes(W, H, want_grad=grad)
    assert nbytes % 4 == 0
    junk = lambda n: np.full(n, NAN_BITS, np.uint32).view(np.float32)
    host = {"x": np.array(x), "y": np.array(y), "scratch": junk(nbytes // 4)}
    if grad:
        host["grad"] = junk(x.size).reshape(x.shape)
    if value:
        host["loss"] = junk(lr.NVALUES)
    d = DevPlanes(torch, host, off=1)
    torch.cuda.synchronize()
    gsr.image_loss(d.ptr["x"], d.ptr["y"], W, H, w_l1=weights[0], w_l2=weights[1], w_dssim=weights[2],
                   grad_scale=grad_scale, grad_ptr=d.ptr.get("grad"), loss_ptr=d.ptr.get("loss"),
                   scratch_ptr=d.ptr["scratch"], scratch_bytes=nbytes, stream=stream)
    torch.cuda.synchronize()
    out = d.host()                                           # asserts every guard word
    assert same_bits(out["x"], x) and same_bits(out["y"], y), "an input was written"
    return out.get("grad"), out.get("loss")


def assert_close(case, weights, got_grad, got_vals, scale=1.0):
    r = lr.reference(case, weights)
    what = f"{case} {weights}"
    if got_grad is not None:
        want = scale * r["grad"]
        err = float(np.abs(got_grad.astype(np.float64) - want).max())
        tol = MARGIN * max(E32[r["content"]], EPS) * scale * r["A"]
        print(f"{what}: gradient error {err:.3g} (/A {err / (scale * r['A']) if r['A'] else 0:.3g}), bound {tol:.3g}")
        assert np.isfinite(got_grad).all(), what
        assert err <= tol, f"{what}: gradient error {err} > {tol}"
    if got_vals is not None:
        for k in range(lr.NVALUES):
            err = abs(float(got_vals[k]) - r["values"][k])
            tol = MARGIN * max(EL32, EPS * abs(r["values"][k]))
            assert err <= tol, f"{what}: loss value {k} = {got_vals[k]}, want {r['values'][k]} (error {err} > {tol})"


# ---------------------------------------------------------------- 1. against the reference

@pytest.mark.parametrize("case", list(lr.CASES))
def test_against_reference(gpu, torch, case):
    r0 = lr.reference(case, lr.WEIGHTINGS[0])
    for weights in lr.WEIGHTINGS:
        g, v = run(gpu, torch, r0["x"], r0["y"], weights)
        assert_close(case, weights, g, v)


@pytest.mark.parametrize("case", [c for c in lr.CASES if c.startswith("equal")])
def test_equal_images_have_exactly_zero_gradient(gpu, torch, case):
    r = lr.reference(case, lr.WEIGHTINGS[0])
    for weights in ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0)):
        g, v = run(gpu, torch, r["x"], r["y"], weights)
        assert not g.any(), f"{case} {weights}"
        assert v[0] == 0 and v[1] == 0 and v[2] == 0


# ---------------------------------------------------------------- 2. modes

MODE_CASES = ["rand-37x29", "bright-130x33", "zero-17x17", "close-300x1", "rand-1x1"]


@pytest.mark.parametrize("case", MODE_CASES)
def test_value_only_and_gradient_only_give_the_combined_bits(gpu, torch, case):
    r = lr.reference(case, lr.WEIGHTINGS[0])
    for weights in (lr.WEIGHTINGS[0], (0.3, 0.5, 0.2)):
        g, v = run(gpu, torch, r["x"], r["y"], weights)
        g_only, none = run(gpu, torch, r["x"], r["y"], weights, value=False)
        assert none is None and same_bits(g_only, g)
        none, v_only = run(gpu, torch, r["x"], r["y"], weights, grad=False)
        assert none is None and same_bits(v_only, v)


@pytest.mark.parametrize("case", MODE_CASES)
def test_grad_scale(gpu, torch, case):
    weights = lr.WEIGHTINGS[0]
    r = lr.reference(case, weights)
    _, v1 = run(gpu, torch, r["x"], r["y"], weights)
    for scale in (0.25, 0.0):
        g, v = run(gpu, torch, r["x"], r["y"], weights, grad_scale=scale)
        assert same_bits(v, v1), "the loss values depend on grad_scale"
        if scale == 0.0:
            assert not g.any()
        else:
            assert_close(case, weights, g, None, scale=scale)


def test_two_streams_give_the_same_bits(gpu, torch):
    r = lr.reference("close-130x33", lr.WEIGHTINGS[0])
    runs = []
    for _ in range(2):
        s = torch.cuda.Stream()
        runs.append(run(gpu, torch, r["x"], r["y"], lr.WEIGHTINGS[0], stream=s.cuda_stream))
    assert same_bits(runs[0][0], runs[1][0]) and same_bits(runs[0][1], runs[1][1])
    again = run(gpu, torch, r["x"], r["y"], lr.WEIGHTINGS[0])
    assert same_bits(again[0], runs[0][0]) and same_bits(again[1], runs[0][1])


def test_more_tiles_than_workgroups(gpu, torch):
    """640 x 360: 2,760 tiles over the 2,048 workgroups the tiled launches are capped at, so
    some workgroups walk two tiles (and most one).  Against the float32 reference's own
    figures: a `rand` image at another size, same bounds."""
    W, H = 640, 360
    rng = np.random.default_rng(640)
    x, y = rng.random((3, H, W)).astype(np.float32), rng.random((3, H, W)).astype(np.float32)
    weights = lr.WEIGHTINGS[0]
    vals, grad = lr.evaluate(x, y, weights)
    g, v = run(gpu, torch, x, y, weights)
    A = float(np.abs(grad).max())
    err = float(np.abs(g.astype(np.float64) - grad).max())
    print(f"640x360: gradient error / A {err / A:.3g}")
    assert err <= MARGIN * max(E32["rand"], EPS) * A
    for k in range(lr.NVALUES):
        assert abs(float(v[k]) - vals[k]) <= MARGIN * max(EL32, EPS * abs(vals[k]))


# ---------------------------------------------------------------- 3. the closed loop

W = H = 64


def test_descent_with_the_image_loss(gpu, torch):
    """test_gpu_adam.test_descent with the loss on the device: re-fitting sh_dc and the
    opacities to the scene's own render from a perturbed start, render -> image_loss(0.8, 0,
    0.2) -> render_backward_scene -> adam_step.  The loss must fall and the frozen arrays keep
    their bits.  Nothing tighter is asserted: any figure would be measured against the code
    under test."""
    soa = dense_soa()
    n = soa.shape[1]
    cam = cam_for(gpu, W, H, **CAMS[0])
    r = exact_renderer(gpu)
    target = dev(torch, frame(gpu, torch, r, gpu.Scene.from_soa(soa), cam, W, H).reshape(-1))
    rng = np.random.default_rng(9)
    start = soa.copy()
    start[11:14] += rng.normal(0, 0.2, (3, n)).astype(np.float32)
    start[3] *= np.float32(0.7)
    scene = gpu.Scene.from_soa(start)
    g, m, v = (zeros_like_groups(torch, n, ("opacity", "sh")) for _ in range(3))
    image = torch.zeros(3 * W * H, dtype=torch.float32, device="cuda")
    grad = torch.zeros(3 * W * H, dtype=torch.float32, device="cuda")
    loss = torch.zeros(lr.NVALUES, dtype=torch.float32, device="cuda")
    scratch = torch.zeros(gpu.image_loss_scratch_bytes(W, H) // 4, dtype=torch.float32, device="cuda")
    assert frame(gpu, torch, r, scene, cam, W, H) is not None   # grows the context's buffers
    first = None
    for it in range(1, 41):
        r.render(scene, cam, W, H, image.data_ptr())
        gpu.image_loss(image, target, W, H, grad_ptr=grad, loss_ptr=loss, scratch_ptr=scratch)
        if first is None:
            first = loss.clone()
        r.render_backward_scene(scene, cam, W, H, grad_image_ptr=grad, opacity_ptr=g["opacity"], sh_ptr=g["sh"])
        scene.adam_step(g, m, v, step=it, lr_sh_dc=0.01, lr_opacity=0.05, zero_grads=True)
        assert r.sync() == 0
    r.render(scene, cam, W, H, image.data_ptr())
    gpu.image_loss(image, target, W, H, loss_ptr=loss, scratch_ptr=scratch)   # value only
    assert r.sync() == 0
    first, last = first.cpu().numpy(), loss.cpu().numpy()
    print(f"descent: L {first[0]:.6g} -> {last[0]:.6g}, MSE {first[2]:.6g} -> {last[2]:.6g}, "
          f"SSIM {first[3]:.6g} -> {last[3]:.6g} after 40 steps")
    assert np.isfinite(first).all() and np.isfinite(last).all()
    assert first[0] > 0 and last[0] < first[0]
    now = scene.download()
    frozen = [a for a in range(38) if a not in (3, 11, 12, 13)]
    assert same_bits(now[frozen], start[frozen])
