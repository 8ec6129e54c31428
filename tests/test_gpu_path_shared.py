"""Shared preprocess of a camera path's frames in flight (GSR_TUNE_PATH_SHARED_PRE,
include/gsr.h): one k_preprocess_multi launch per group of frames reads the scene once and
writes every lane's records, items, rects and spans.  The records are the same bits as
k_preprocess's, so knob on and knob off must give bit-equal images in both blend modes (and
each must pass the oracle rule of its blend mode); the readbacks after a shared path equal
a plain gsr_render's; scenes the shared kernel does not cover fall back to one launch per
frame; the double-buffered outputs hand over correctly across calls, between other entry
points, and after errors."""
import numpy as np
import pytest

from conftest import scene_soa
from test_gpu_parity import assert_image_parity, cam_for
from test_gpu_path import orbit_cams, render_path_checked

pytestmark = pytest.mark.gpu

KNOB, LAUNCHES = 34, 35
W, H = 320, 240


@pytest.fixture(scope="module")
def torch(gpu):
    import torch as t
    assert t.cuda.is_available()
    return t


@pytest.fixture(scope="module")
def c1(gpu, tmp_path_factory):
    return scene_soa(gpu, tmp_path_factory, 10_000, 1)


@pytest.fixture(scope="module")
def want8(gpu, orc, c1):
    """The oracle's images of the eight orbit cameras over config 1, computed once."""
    return [orc.render(c1[1], cam, W, H, 3.0) for cam in orbit_cams(gpu, W, H, 8)]


def multi_launches(F, m):
    """k_preprocess_multi launches of an m-frame call on F lanes: per group of s >= 2 frames,
    one per four cameras and one for a remainder of two or three (a remainder of one, and a
    group of one, go through k_preprocess)."""
    F = min(F, m)
    per = lambda s: 0 if s < 2 else s // 4 + (1 if s % 4 >= 2 else 0)
    return (m // F) * per(F) + per(m % F)


def renderer(gpu, F, shared, exact):
    r = gpu.Renderer()
    r.set_frames_in_flight(F)
    r.set_tuning(KNOB, 1 if shared else 0)
    r.set_tuning(22, 0 if exact else 1)
    return r


def path_images(gpu, torch, r, scene, cams, **kw):
    outs = [torch.full((3 * W * H,), -1.0, device="cuda") for _ in cams]
    render_path_checked(r, scene, cams, W, H, [o.data_ptr() for o in outs], **kw)
    return [o.view(3, H, W).cpu().numpy() for o in outs]


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("F", [2, 3, 4, 8])
def test_shared_equals_per_frame_and_oracle(gpu, torch, c1, want8, F, exact):
    scene = gpu.Scene.from_soa(c1[1])
    on, off = renderer(gpu, F, True, exact), renderer(gpu, F, False, exact)
    for m in sorted({1, F - 1, F, F + 1, 2 * F + 1, 4 * F + 3}):
        cams = orbit_cams(gpu, W, H, m)
        before = on.get_tuning(LAUNCHES)
        a = path_images(gpu, torch, on, scene, cams)
        got = on.get_tuning(LAUNCHES) - before
        want = multi_launches(F, m)
        assert got in (want, 2 * want, 3 * want), (F, m, got)   # render_path_checked may render the call again
        b = path_images(gpu, torch, off, scene, cams)
        assert off.get_tuning(LAUNCHES) == 0
        for i in range(m):
            assert np.array_equal(a[i].view(np.uint32), b[i].view(np.uint32)), f"F {F}, {m} frames: frame {i}"
            assert_image_parity(a[i], want8[i % 8], exact=exact)


def splats_equal(a, b):
    """Two read_splats results of the same frame: every rect, key and tile count, and the
    records of the Gaussians that were kept (a culled Gaussian's record is never written)."""
    wa, wb = a.view(np.uint32).reshape(len(a), 16), b.view(np.uint32).reshape(len(b), 16)
    assert np.array_equal(wa[:, 12:16], wb[:, 12:16])
    live = wa[:, 15] != 0xFFFFFFFF
    assert np.array_equal(wa[live], wb[live])
    return int(live.sum())


@pytest.mark.parametrize("F,m", [(4, 11), (2, 5), (8, 16)])
def test_readbacks_after_shared_path(gpu, torch, c1, F, m):
    """Lane 0's last frame: records, rects, keys, depth order and tile lists as a plain render's."""
    n = c1[1].shape[1]
    scene = gpu.Scene.from_soa(c1[1])
    cams = orbit_cams(gpu, W, H, m)
    r = renderer(gpu, F, True, True)
    path_images(gpu, torch, r, scene, cams)
    assert r.get_tuning(LAUNCHES) > 0
    last = max(i for i in range(m) if i % F == 0)
    p = renderer(gpu, 1, False, True)
    out = torch.empty(3 * W * H, device="cuda")
    p.render(scene, cams[last], W, H, out.data_ptr())
    assert p.sync() == 0
    assert splats_equal(r.read_splats(n), p.read_splats(n)) > 100
    assert np.array_equal(r.read_depth_order(n), p.read_depth_order(n))
    assert np.array_equal(r.read_tile_ranges(), p.read_tile_ranges())
    assert np.array_equal(r.read_pairs(), p.read_pairs())


@pytest.mark.parametrize("n", [0, 1, 63, 65, 257, 1000, 4099])
def test_scene_sizes(gpu, orc, torch, c1, n):
    soa = np.ascontiguousarray(c1[1][:, :n])
    scene = gpu.Scene.from_soa(soa)
    cams = orbit_cams(gpu, W, H, 7)
    r = renderer(gpu, 3, True, True)
    imgs = path_images(gpu, torch, r, scene, cams)
    assert (r.get_tuning(LAUNCHES) > 0) == (n > 0)
    for cam, img in zip(cams, imgs):
        assert_image_parity(img, orc.render(soa, cam, W, H, 3.0), exact=True)


def opposite_cams(gpu):
    """Two cameras back to back inside the scene, so each has behind it the Gaussians that the
    other sees, then two orbit cameras."""
    return [cam_for(gpu, W, H, pos=(0.0, 0.0, 0.1), look=(0.0, 0.0, -3.0)),
            cam_for(gpu, W, H, pos=(0.0, 0.0, -0.1), look=(0.0, 0.0, 3.0)), *orbit_cams(gpu, W, H, 2)]


def test_cameras_cull_independently(gpu, orc, torch, c1):
    soa = c1[1]
    n = soa.shape[1]
    scene = gpu.Scene.from_soa(soa)
    cams = opposite_cams(gpu)
    st = [orc.preprocess(soa, cam, W, H, 3.0)["status"] == 2 for cam in cams[:2]]
    assert (st[0] & ~st[1]).sum() > 50 and (st[1] & ~st[0]).sum() > 50, "the cameras do not cull different Gaussians"
    r = renderer(gpu, 4, True, True)
    imgs = path_images(gpu, torch, r, scene, cams)
    assert r.get_tuning(LAUNCHES) > 0
    for cam, img in zip(cams, imgs):
        assert_image_parity(img, orc.render(soa, cam, W, H, 3.0), exact=True)
    # lane 1's camera through the path's lane 0: a one-lane renderer, the same records
    for j in (0, 1):
        r2 = renderer(gpu, 2, True, True)
        path_images(gpu, torch, r2, scene, [cams[j], cams[1 - j]])
        p = renderer(gpu, 1, False, True)
        out = torch.empty(3 * W * H, device="cuda")
        p.render(scene, cams[j], W, H, out.data_ptr())
        assert p.sync() == 0
        assert splats_equal(r2.read_splats(n), p.read_splats(n)) == st[j].sum()


def test_sh3_scene(gpu, orc, torch, c1):
    """SH-3: the 48 coefficients are loaded late, by the first camera that keeps the Gaussian;
    with the opposite cameras that is camera 0 for some Gaussians and camera 1 for others."""
    path, soa = c1
    scene = gpu.Scene.from_ply(path, sh3=True)
    assert scene.is_sh3
    soa3 = orc.ply_read_sh3(path)
    cams = opposite_cams(gpu) + orbit_cams(gpu, W, H, 5)[2:]
    for F in (2, 4):
        on, off = renderer(gpu, F, True, True), renderer(gpu, F, False, True)
        a = path_images(gpu, torch, on, scene, cams)
        b = path_images(gpu, torch, off, scene, cams)
        assert on.get_tuning(LAUNCHES) > 0 and off.get_tuning(LAUNCHES) == 0
        with orc.sh3_mode():
            for cam, x, y in zip(cams, a, b):
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
                assert_image_parity(x, orc.render(soa3, cam, W, H, 3.0), exact=True)


def test_fallbacks_render_exactly_without_shared_launches(gpu, orc, torch, c1, want8, tmp_path_factory):
    from gaussianrenderer_amd import _native
    from test_gpu_parity import aos_records
    soa = c1[1]
    cams = orbit_cams(gpu, W, H, 7)
    # a 4D scene with times
    p = tmp_path_factory.mktemp("shared4d") / "scene4d.ply"
    gpu.write_synthetic_ply4d(str(p), 5_000, 5)
    soa49 = gpu.read_ply(str(p), four_d=True)
    s4 = gpu.Scene.from_ply(str(p))
    times = [0.0, 0.2, 0.4, 0.55, 0.7, 0.85, 1.0]
    r = renderer(gpu, 3, True, True)
    imgs = path_images(gpu, torch, r, s4, [cams[0]] * 7, times=times)
    assert r.get_tuning(LAUNCHES) == 0
    for t, img in zip(times, imgs):
        assert_image_parity(img, orc.render(orc.temporal(soa49, t), cams[0], W, H, 3.0), exact=True)
    # AoS input
    dev = torch.from_numpy(aos_records(soa)).cuda()
    r = renderer(gpu, 3, True, True)
    imgs = path_images(gpu, torch, r, dev.data_ptr(), cams, layout=_native.LAYOUT_AOS, n=soa.shape[1])
    assert r.get_tuning(LAUNCHES) == 0
    for i, img in enumerate(imgs):
        assert_image_parity(img, want8[i], exact=True)
    # forced depth split, and diagnostics
    scene = gpu.Scene.from_soa(soa)
    for prepare in (lambda r: r.set_tuning(gpu.TUNE_DEPTH_SPLIT, 1), lambda r: r.set_diagnostics(True)):
        r = renderer(gpu, 3, True, True)
        prepare(r)
        imgs = path_images(gpu, torch, r, scene, cams)
        assert r.get_tuning(LAUNCHES) == 0
        for i, img in enumerate(imgs):
            assert_image_parity(img, want8[i], exact=True)


@pytest.mark.parametrize("F,chunk,calls", [(4, 5, 3), (4, 3, 2), (3, 7, 3), (2, 2, 3)])
def test_chained_calls_without_join(gpu, torch, c1, want8, F, chunk, calls):
    """The multi-GPU frame loop's calls (frame events, no exit join) over a ring of `chunk`
    buffers, shorter and longer than the lanes: a call's first shared launch overwrites the
    set the lanes' frames of two groups back used, which may still be running."""
    scene = gpu.Scene.from_soa(c1[1])
    cams = orbit_cams(gpu, W, H, chunk * calls)
    r = renderer(gpu, F, True, True)
    warm = [torch.empty(3 * W * H, device="cuda") for _ in range(4 * 8)]
    render_path_checked(r, scene, [orbit_cams(gpu, W, H, 8)[(i // F) % 8] for i in range(4 * 8)], W, H,
                        [w.data_ptr() for w in warm])
    torch.cuda.synchronize()
    bufs = [torch.empty(3 * W * H, device="cuda") for _ in range(chunk)]
    evs = [torch.cuda.Event() for _ in range(chunk)]
    S = torch.cuda.current_stream()
    cons = torch.cuda.Stream()
    snaps = []
    before = r.get_tuning(LAUNCHES)
    for c in range(calls):
        S.wait_stream(cons)
        rc = r.render_path(scene, cams[c * chunk:(c + 1) * chunk], W, H, [b.data_ptr() for b in bufs], events=evs,
                           join=False, stream=S.cuda_stream)
        assert rc == 0
        with torch.cuda.stream(cons):
            for j in range(chunk):
                cons.wait_event(evs[j])
                snaps.append(bufs[j].clone())
    torch.cuda.synchronize()
    assert r.sync() == 0
    assert r.get_tuning(LAUNCHES) - before == calls * multi_launches(F, chunk)
    for i, snap in enumerate(snaps):
        assert_image_parity(snap.view(3, H, W).cpu().numpy(), want8[i % 8], exact=True)


def test_other_entry_points_between_path_calls(gpu, orc, torch, c1, want8):
    soa = c1[1]
    n = soa.shape[1]
    scene = gpu.Scene.from_soa(soa)
    cams = orbit_cams(gpu, W, H, 8)
    r = renderer(gpu, 4, True, True)
    ref = renderer(gpu, 1, False, True)
    out = torch.empty(3 * W * H, device="cuda")

    def path():
        for i, img in enumerate(path_images(gpu, torch, r, scene, cams)):
            assert_image_parity(img, want8[i], exact=True)

    path()
    r.render(scene, cams[3], W, H, out.data_ptr())
    assert r.sync() == 0
    assert_image_parity(out.view(3, H, W).cpu().numpy(), want8[3], exact=True)
    path()
    alpha = [torch.empty(W * H, device="cuda") for _ in range(2)]
    for x, a in zip((r, ref), alpha):
        x.render_aux(scene, cams[5], W, H, out_ptr=out.data_ptr(), alpha_ptr=a.data_ptr())
        assert x.sync() == 0
        assert_image_parity(out.view(3, H, W).cpu().numpy(), want8[5], exact=True)
    assert torch.equal(alpha[0], alpha[1])
    path()
    count = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2)]
    for x, cnt in zip((r, ref), count):
        x.render_contrib(scene, cams[6], W, H, count_ptr=cnt.data_ptr())
        assert x.sync() == 0
    assert torch.equal(count[0], count[1]) and int(count[0].sum()) > 0
    path()
    assert r.get_tuning(LAUNCHES) >= 8


@pytest.mark.parametrize("fail", [4, 6, 7, 8])
def test_failed_frame_leaves_earlier_frames_complete(gpu, torch, c1, want8, fail):
    """GSR_TUNE_FAIL_FRAME at the first (4, 8), a middle (6) and the last (7) frame of a group of
    four: the frames before it, those of its own group included, are complete and joined to
    the caller's stream; the frames from it on are not rendered; the next call is exact."""
    scene = gpu.Scene.from_soa(c1[1])
    cams = orbit_cams(gpu, W, H, 11)
    r = renderer(gpu, 4, True, True)
    s = torch.cuda.Stream()
    outs = [torch.empty(3 * W * H, device="cuda") for _ in cams]
    ptrs = [o.data_ptr() for o in outs]
    render_path_checked(r, scene, cams, W, H, ptrs, stream=s.cuda_stream)
    with torch.cuda.stream(s):
        for o in outs:
            o.fill_(float("nan"))
    r.set_tuning(gpu.TUNE_FAIL_FRAME, fail)
    with pytest.raises(gpu.GsrError):
        r.render_path(scene, cams, W, H, ptrs, stream=s.cuda_stream)
    with torch.cuda.stream(s):
        snap = torch.stack(outs).clone()
    s.synchronize()
    for i in range(len(cams)):
        img = snap[i].view(3, H, W).cpu().numpy()
        if i < fail:
            assert_image_parity(img, want8[i % 8], exact=True)
        else:
            assert np.isnan(img).all(), f"frame {i} was rendered after frame {fail} failed"
    torch.cuda.synchronize()
    assert r.sync() == 0
    for i, img in enumerate(path_images(gpu, torch, r, scene, cams, stream=s.cuda_stream)):
        assert_image_parity(img, want8[i % 8], exact=True)


def test_pair_overflow_on_child_lane(gpu, orc, torch):
    """Huge splats overflow every lane's initial pair buffer under the shared launch: the call
    (or the sync) reports it, the lanes grow, and the re-rendered path is exact."""
    n = 3000
    rng = np.random.default_rng(9)
    soa = np.zeros((38, n), np.float32)
    soa[0:3] = rng.uniform(-0.2, 0.2, (3, n))
    soa[3] = rng.uniform(0.01, 0.05, n)
    soa[4:7] = rng.uniform(1.0, 2.0, (3, n))
    soa[7] = 1.0
    soa[11:38] = rng.normal(0, 0.3, (27, n))
    BW, BH = 640, 480
    cams = orbit_cams(gpu, BW, BH, 3)
    scene = gpu.Scene.from_soa(soa)
    r = renderer(gpu, 3, True, True)
    outs = [torch.empty(3 * BW * BH, device="cuda") for _ in cams]
    ptrs = [o.data_ptr() for o in outs]
    rc = r.render_path(scene, cams, BW, BH, ptrs)
    assert rc == -5 or r.sync() == -5
    render_path_checked(r, scene, cams, BW, BH, ptrs)
    assert r.get_tuning(LAUNCHES) >= 2
    for cam, o in zip(cams, outs):
        assert_image_parity(o.view(3, BH, BW).cpu().numpy(), orc.render(soa, cam, BW, BH, 3.0), exact=True)
