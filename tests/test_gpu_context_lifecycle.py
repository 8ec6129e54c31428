"""A context's whole workspace through its life: every buffer a context can own is allocated
by ordinary API calls, the per-Gaussian ones are outgrown and reallocated once, the context is
destroyed, and a context created after it renders the same frame bit for bit, within the
oracle gate.  Values only: nothing here looks at freed memory or at the device's free memory."""
import numpy as np
import pytest

from test_gpu_parity import assert_image_parity, c1, cam_for  # noqa: F401 (c1: fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch(gpu):
    import torch as t
    assert t.cuda.is_available()
    return t

W, H = 160, 120
N_SMALL, N_LARGE = 1000, 4000   # below and above the 1,024-element floor of the per-Gaussian buffers


def test_context_lifecycle(gpu, orc, torch, c1):  # noqa: F811
    _, soa = c1
    small = gpu.Scene.from_soa(soa[:, :N_SMALL])
    large = gpu.Scene.from_soa(soa[:, :N_LARGE])
    cam = cam_for(gpu, W, H)
    cams = [cam_for(gpu, W, H, pos=(0.3 * i - 0.7, 0.1 * i, 4.0 - 0.2 * i)) for i in range(6)]
    dev = dict(device="cuda")
    image = torch.empty(3 * W * H, dtype=torch.float32, **dev)

    def plain(r, scene):
        """One plain frame; a context's first frame may report the documented first-frame
        overflow (tests/test_gpu_parity.py test_depth_pass_budget_adapts_and_recovers)."""
        for _ in range(3):
            r.render(scene, cam, W, H, image.data_ptr())
            if r.sync() == 0:
                break
        assert r.sync() == 0
        return image.view(3, H, W).cpu().numpy()

    a = gpu.Renderer()
    a.set_tuning(gpu.TUNE_BLEND_EXP, 0)
    a.set_frames_in_flight(3)
    a.set_diagnostics(True)                   # the blend counters and take map
    a.set_tuning(gpu.TUNE_DEPTH_SPLIT, 1)     # forced: the split buffers, at this small size too
    plain(a, small)
    plain(a, small)                           # key mode (a threshold exists): the preprocess-order buffer
    want_a = plain(a, large).copy()           # every per-Gaussian buffer outgrown and reallocated
    assert a.get_tuning(gpu.TUNE_DEPTH_SPLIT_STATE) != 0   # the frame was split

    # a camera path: the lanes, and (its frames share one preprocess launch only with the split
    # and the diagnostics off) each lane's second set of preprocess outputs
    a.set_diagnostics(False)
    a.set_tuning(gpu.TUNE_DEPTH_SPLIT, 0)
    outs = [torch.empty(3 * W * H, dtype=torch.float32, **dev) for _ in range(3)]
    a.render_path(large, cams, W, H, [outs[i % 3].data_ptr() for i in range(6)])
    assert a.sync() == 0
    assert a.get_tuning(gpu.TUNE_PATH_SHARED_LAUNCHES) > 0
    for i in (3, 4, 5):   # the last writer of each output
        assert_image_parity(outs[i % 3].view(3, H, W).cpu().numpy(),
                            orc.render(soa[:, :N_LARGE], cams[i], W, H, 3.0), exact=True)

    # an aux frame with a depth target and more than four features (the -Z array, the feature pack)
    nfeat = 5
    feats = torch.rand(nfeat * N_LARGE, dtype=torch.float32, **dev)
    depth = torch.empty(W * H, dtype=torch.float32, **dev)
    fout = torch.empty(nfeat * W * H, dtype=torch.float32, **dev)
    a.render_aux(large, cam, W, H, out_ptr=image.data_ptr(), depth_ptr=depth.data_ptr(),
                 features_ptr=feats.data_ptr(), nfeat=nfeat, feat_out_ptr=fout.data_ptr())
    assert a.sync() == 0
    assert np.array_equal(image.view(3, H, W).cpu().numpy().view(np.uint32), want_a.view(np.uint32))
    assert bool(torch.isfinite(depth).all()) and bool(torch.isfinite(fout).all()) and float(fout.abs().sum()) > 0

    count = torch.zeros(N_LARGE, dtype=torch.int32, **dev)
    a.render_contrib(large, cam, W, H, count_ptr=count.data_ptr())
    assert a.sync() == 0
    assert int(count.sum()) > 0

    # the whole backward pass without a caller's scratch (the context's ten gradient planes)
    grad_image = torch.ones(3 * W * H, dtype=torch.float32, **dev)
    g_opacity = torch.zeros(N_LARGE, dtype=torch.float32, **dev)
    a.render_backward_scene(large, cam, W, H, grad_image_ptr=grad_image, opacity_ptr=g_opacity)
    assert a.sync() == 0
    assert bool(torch.isfinite(g_opacity).all()) and float(g_opacity.abs().sum()) > 0
    a.close()

    b = gpu.Renderer()
    b.set_tuning(gpu.TUNE_BLEND_EXP, 0)
    got_b = plain(b, large)
    b.close()
    assert np.array_equal(got_b.view(np.uint32), want_a.view(np.uint32))
    assert_image_parity(got_b, orc.render(soa[:, :N_LARGE], cam, W, H, 3.0), exact=True)
