"""The blend family takes the same decisions: one frame through k_blend_w (the exact blend),
k_blend_aux, k_blend_contrib and k_blend_backward, compared with each other on the GPU.

The four kernels walk a block's list with one set of functions (csrc/gsr_blend_device.h:
block_cull, ballot_rank, splat_step, and for the derived passes block_setup, batch_first and
batch_prefetch), so each derived pass adds to exactly the splats the image composited.  The
other blend tests pin each kernel to the CPU oracle (test_gpu_parity.py, test_gpu_aux.py,
test_gpu_contrib.py, test_gpu_backward.py); none compares the kernels with each other, which
is what a cull or step changed in one kernel alone would break first.

Scene: the 200 dense Gaussians of test_gpu_contrib.py at 37 x 23, plain and with a tiling
that covers 30 x 18 of it.  Every tile lists up to all 200 records: three full 64-record
batches and a partial one (both prefetch distances and the cnt < 64 tail), and the sizes
leave blocks partly outside the image and partly outside the cover."""
import numpy as np
import pytest

from conftest import KNOB_BLEND_EXP
from test_gpu_aux import aux
from test_gpu_contrib import contrib, dense_soa, same_bits, tiling_of
from test_gpu_parity import cam_for

pytestmark = pytest.mark.gpu

W, H = 37, 23
CASES = {"plain": None, "partial": (3, 2, 10, 9)}   # cover 30 x 18


@pytest.fixture(scope="module")
def torch(gpu):
    import torch as t
    assert t.cuda.is_available()
    return t


@pytest.fixture(scope="module")
def scene(gpu):
    return gpu.Scene.from_soa(dense_soa())


_frames = {}


def frame(gpu, torch, scene, case):
    """The four kernels' outputs for one case, computed once: the exact blend's image and take
    counts (diagnostics), the aux colour planes, the contrib count and weight, and the
    backward colour gradient for g_image = 1 on the red plane."""
    if case not in _frames:
        tiling = CASES[case]
        cam = cam_for(gpu, W, H)
        n = scene.n
        r = gpu.Renderer()
        r.set_tuning(KNOB_BLEND_EXP, 0)

        def exact():
            out = torch.full((3, H, W), float("nan"), dtype=torch.float32, device="cuda")
            for _ in range(3):
                r.render(scene, cam, W, H, out.data_ptr(), tiling=tiling_of(gpu, W, H, tiling))
                if r.sync() == 0:
                    return out.cpu().numpy()
            raise AssertionError("frame still incomplete after three renders")

        img = exact()
        r.set_diagnostics(True)
        img_d = exact()
        takes = r.take_map(W, H) & np.uint64(0xFFFFFFFF)
        r.set_diagnostics(False)
        assert same_bits(img, img_d)   # the take map describes the shipped kernel's composite

        colour = aux(gpu, torch, scene, cam, W, H, alpha=False, depth=False, tiling=tiling, renderer=r)["out"]
        stats = contrib(gpu, torch, scene, cam, W, H, what="cw", tiling=tiling, renderer=r)

        g = torch.zeros((3, H, W), dtype=torch.float32, device="cuda")
        g[0] = 1.0
        grad = torch.zeros((3, n), dtype=torch.float32, device="cuda")
        for attempt in range(3):
            grad.zero_()
            r.render_backward(scene, cam, W, H, grad_image_ptr=g, color_ptr=grad,
                              tiling=tiling_of(gpu, W, H, tiling))
            if r.sync() == 0:
                break
        else:
            raise AssertionError("backward frame still incomplete after three renders")

        f = {"img": img, "takes": takes, "colour": colour, "count": stats["count"], "weight": stats["weight"],
             "grad": grad.cpu().numpy()}
        for v in f.values():
            v.setflags(write=False)
        _frames[case] = f
    return _frames[case]


@pytest.mark.parametrize("case", list(CASES))
def test_aux_colours_are_the_exact_image(gpu, torch, scene, case):
    f = frame(gpu, torch, scene, case)
    assert same_bits(f["colour"], f["img"])


@pytest.mark.parametrize("case", list(CASES))
def test_contrib_counts_sum_to_the_take_map(gpu, torch, scene, case):
    f = frame(gpu, torch, scene, case)
    total = int(f["count"].astype(np.uint64).sum())
    print("takes", total, "per pixel up to", int(f["takes"].max()), "Gaussians taken", int((f["count"] > 0).sum()))
    assert total > 0
    assert total == int(f["takes"].sum())


@pytest.mark.parametrize("case", list(CASES))
def test_backward_red_gradient_is_the_contrib_weight(gpu, torch, scene, case):
    """dL/d red_i = sum over takes of w = alpha T, the weight contrib sums.  Contrib rounds
    each w to 2^-24 fixed point (at most 2^-25 off per take); backward adds count_i floats in
    an order that is not fixed (n u sum|x|, u = 2^-24)."""
    f = frame(gpu, torch, scene, case)
    count = f["count"].astype(np.float64)
    wsum = f["weight"].astype(np.float64) / 2.0 ** 24
    red = f["grad"][0].astype(np.float64)
    bound = count * 2.0 ** -25 + count * 2.0 ** -24 * wsum
    err = np.abs(red - wsum)
    worst = int(np.argmax(err - bound))
    print("worst Gaussian", worst, "error", err[worst], "bound", bound[worst])
    assert (err <= bound).all(), (worst, red[worst], wsum[worst], bound[worst])
    assert (f["grad"][0][f["count"] == 0] == 0.0).all()
    assert (f["grad"][1:] == 0.0).all()   # g_image is 0 on the green and blue planes
