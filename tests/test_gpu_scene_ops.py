"""Device-side scene editing (gsr_mask_indices, gsr_gather_planes, gsr_scene_gather,
gsr_scene_select; Scene.select / Scene.gather, mask_indices, gather_planes): the index lists
and the gathered planes against numpy exactly, and the property that makes the feature worth
having: a selection keeps index order, the depth sort's tie-break, so dropping the Gaussians
no pixel composited (render_contrib's count == 0) leaves the exact blend's image, the
oracle's, bit for bit unchanged."""
import ctypes

import numpy as np
import pytest

from conftest import scene_soa
from test_gpu_aux import random_soa
from test_gpu_parity import CAMS, cam_for

pytestmark = pytest.mark.gpu

# the implementation's compaction geometry (gsr_scene_ops.hip): mask bytes per workgroup, and
# chunk counts the single scan workgroup takes per iteration
MASK_CHUNK = 4096
MASK_SCAN_TILE = 1024
KNOB_BLEND_EXP = 22
SENT32, SENT64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31


@pytest.fixture(scope="module")
def torch(gpu):
    import torch as t
    assert t.cuda.is_available()
    return t


@pytest.fixture(scope="module")
def c1(gpu, tmp_path_factory):
    return scene_soa(gpu, tmp_path_factory, 10_000, 1)


@pytest.fixture(scope="module")
def scene1(gpu, c1):
    return gpu.Scene.from_soa(c1[1])


def dense_soa():
    """test_gpu_contrib.dense_soa's recipe with n = 600."""
    rng = np.random.default_rng(22); n = 600
    soa = np.zeros((38, n), np.float32)
    soa[0:3] = rng.uniform(-0.5, 0.5, (3, n)); soa[3] = rng.uniform(0.5, 0.99, n)
    soa[4:7] = rng.uniform(0.1, 0.4, (3, n)); soa[7] = 1.0
    soa[11:38] = rng.normal(0, 0.3, (27, n))
    return soa


@pytest.fixture(scope="module")
def dense(gpu):
    soa = dense_soa()
    return soa, gpu.Scene.from_soa(soa)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def dev(torch, a):
    """A host array on the device, bits unchanged (torch has no unsigned 32 / 64-bit dtypes)."""
    a = np.ascontiguousarray(a)
    signed = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype)
    return torch.from_numpy(a.view(signed) if signed else a).cuda()


# ---------------------------------------------------------------- 1. compaction

def masks_for(n, rng):
    nz = rng.choice(np.array([1, 2, 0x80, 0xFF], np.uint8), n)   # non-zero bytes are not only 1
    first, last = np.zeros(n, bool), np.zeros(n, bool)
    first[0] = last[-1] = True
    pats = {"zeros": np.zeros(n, bool), "ones": np.ones(n, bool), "first": first, "last": last,
            "half": rng.random(n) < 0.5, "sparse": rng.random(n) < 0.01}
    return {k: np.where(v, nz, 0).astype(np.uint8) for k, v in pats.items()}


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4095, 4096, 4097, 100_003, MASK_CHUNK * MASK_SCAN_TILE + 3 * MASK_CHUNK + 5])
def test_mask_indices(gpu, torch, n):
    """The last size takes the scan workgroup through a second iteration (more than
    MASK_CHUNK x MASK_SCAN_TILE items).  Every mask also runs from an address that is not
    16-byte aligned (the byte path of the mask loads)."""
    rng = np.random.default_rng(n)
    for name, mask in masks_for(n, rng).items():
        want = np.flatnonzero(mask).astype(np.int32)
        for shift in (0, 1):
            buf = torch.zeros(n + 16, dtype=torch.uint8, device="cuda")
            d_mask = buf[shift:shift + n]
            d_mask.copy_(torch.from_numpy(mask))
            assert d_mask.data_ptr() % 16 == shift
            d_idx = torch.full((n,), -7, dtype=torch.int32, device="cuda")
            m = gpu.mask_indices(d_mask, n, d_idx)
            got = d_idx.cpu().numpy()
            assert m == want.size, (name, shift, m, want.size)
            assert np.array_equal(got[:m], want), (name, shift)
            assert (got[m:] == -7).all(), (name, shift)


# ---------------------------------------------------------------- 2. gather_planes

def special_bits(dtype):
    """-0.0, denormals, quiet and signalling NaNs with payloads, infinities: a copy that went
    through float arithmetic would change some of them."""
    if dtype == np.uint32:
        return np.array([0x80000000, 0x00000001, 0x807FFFFF, 0x7FC12345, 0xFFC00001, 0x7F800001, 0x7F800000,
                         0xFF800000, 0x00000000, 0xFFFFFFFF], np.uint32)
    return np.array([0x8000000000000000, 0x0000000000000001, 0x800FFFFFFFFFFFFF, 0x7FF8000000012345,
                     0xFFF8000000000001, 0x7FF0000000000001, 0x7FF0000000000000, 0xFFFFFFFFFFFFFFFF], np.uint64)


def plane_source(rng, dtype, nplanes, stride):
    src = rng.integers(0, np.iinfo(dtype).max, (nplanes, stride), dtype=dtype, endpoint=True)
    sp = special_bits(dtype)
    src[:, :sp.size] = sp          # stride >= 10 in every case below
    return src


def run_gather(gsr, torch, src, n, idx, dst_stride, bad=None):
    """gather_planes of the (nplanes, src_stride) host array into a sentinel-filled
    (nplanes, dst_stride) device array; returns it on the host."""
    nplanes, src_stride = src.shape
    eb = src.dtype.itemsize
    d_src = dev(torch, src)
    d_idx = dev(torch, np.asarray(idx, np.int32))
    d_dst = torch.full((nplanes, dst_stride), SENT32 if eb == 4 else SENT64,
                       dtype=torch.int32 if eb == 4 else torch.int64, device="cuda")
    gsr.gather_planes(d_dst, dst_stride, d_src, src_stride, nplanes, eb, n, d_idx, len(idx), bad_ptr=bad)
    torch.cuda.synchronize()
    return d_dst.cpu().numpy().view(src.dtype)


@pytest.mark.parametrize("nplanes", [1, 3, 9])
@pytest.mark.parametrize("dtype", [np.uint32, np.uint64])
def test_gather_planes(gpu, torch, dtype, nplanes):
    n = 777
    rng = np.random.default_rng(nplanes * 8 + np.dtype(dtype).itemsize)
    src = plane_source(rng, dtype, nplanes, n + 5)
    sent = dtype(SENT32 if dtype == np.uint32 else SENT64)
    for m in (1, 63, 64, 65, n, 2 * n + 7):
        idx = rng.permutation(n) if m == n else rng.integers(0, n, m)
        k = min(m, 8)
        idx[:k] = np.arange(k)                     # the special values' slots are read
        got = run_gather(gpu, torch, src, n, idx, m + 3)
        assert np.array_equal(got[:, :m], src[:, idx]), m
        assert (got[:, m:] == sent).all(), m


@pytest.mark.parametrize("dtype", [np.uint32, np.uint64])
def test_gather_planes_out_of_range_indices(gpu, torch, dtype):
    """The guarded path: an index outside [0, n) reads element 0 (negative) or n - 1, and
    *d_bad counts them; every other slot is exact."""
    n, m, nplanes = 500, 700, 3
    rng = np.random.default_rng(5)
    src = plane_source(rng, dtype, nplanes, n + 2)
    idx = rng.integers(0, n, m).astype(np.int64)
    where = rng.choice(m, 40, replace=False)
    idx[where] = np.tile([-1, n, INT32_MAX, INT32_MIN], 10)
    idx[[0, 63, 64, m - 1]] = [-1, INT32_MIN, n, INT32_MAX]          # wave edges too
    nbad = int(((idx < 0) | (idx >= n)).sum())
    assert nbad >= 40
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = run_gather(gpu, torch, src, n, idx, m, bad=bad)
    assert int(bad.item()) == nbad
    assert np.array_equal(got, src[:, np.clip(idx, 0, n - 1)])
    # without a counter the same elements arrive
    assert np.array_equal(run_gather(gpu, torch, src, n, idx, m), got)


# ---------------------------------------------------------------- 3. scene_gather / scene_select

def soa_of_kind(gsr, tmp_path_factory, narrays, n=1000):
    d = tmp_path_factory.mktemp(f"ops{narrays}")
    p = str(d / "s.ply")
    if narrays == 49:
        gsr.write_synthetic_ply4d(p, n, 5)
        return gsr.read_ply(p, four_d=True)
    if narrays == 59:
        gsr.write_synthetic_ply(p, n, 11)
        return gsr.read_ply(p, sh3=True)
    return scene_soa(gsr, tmp_path_factory, n, 3)[1]


def header_of(gsr, torch, scene):
    """The block's header words, through gsr_scene_copy (which checks the header against
    (narrays, n) itself) into a device buffer."""
    nbytes = gsr.lib().gsr_scene_bytes(scene.narrays, scene.n)
    assert nbytes == 256 + 4 * scene.narrays * ((scene.n + 63) // 64 * 64)
    buf = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    assert gsr.lib().gsr_scene_copy(buf.data_ptr(), scene.ptr, scene.narrays, scene.n, None) == 0
    torch.cuda.synchronize()
    return buf[:256].cpu().numpy().view(np.uint32)


def assert_header(gsr, torch, scene, narrays, m):
    assert (scene.narrays, scene.n, scene.owned) == (narrays, m, True)
    h = header_of(gsr, torch, scene)
    assert list(h[:4]) == [0x7FC0A5E1, 0x7FC05352, 0x7FC03347, 0x7FC00001]
    assert list(h[4:10].view(np.uint64)) == [m, (m + 63) // 64 * 64, narrays]
    assert not h[10:].any()


@pytest.mark.parametrize("narrays", [38, 49, 59])
def test_scene_gather_and_select(gpu, torch, tmp_path_factory, narrays):
    n = 1000                                           # stride 1024 != n
    soa = soa_of_kind(gpu, tmp_path_factory, narrays, n)
    assert soa.shape == (narrays, n)
    scene = gpu.Scene.from_soa(soa)
    rng = np.random.default_rng(narrays)

    for idx in (rng.permutation(n), rng.integers(0, n, 1500), np.array([n - 1]), np.array([], np.int64)):
        m = len(idx)
        d_idx = dev(torch, idx.astype(np.int32)) if m else None
        g = scene.gather(d_idx, m)
        torch.cuda.synchronize()
        got = g.download()
        assert got.shape == (narrays, m)
        assert same_bits(got, soa[:, idx]), m
        assert_header(gpu, torch, g, narrays, m)
        assert (g.is_4d, g.is_sh3) == (scene.is_4d, scene.is_sh3)

    for mask in (rng.random(n) < 0.5, np.zeros(n, bool), np.ones(n, bool)):
        d_keep = dev(torch, np.where(mask, 0x80, 0).astype(np.uint8))
        d_idx = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        s = scene.select(d_keep, d_idx)
        m = int(mask.sum())
        assert_header(gpu, torch, s, narrays, m)
        got = s.download()
        assert got.shape == (narrays, m)
        assert same_bits(got, soa[:, mask])
        idx = d_idx.cpu().numpy()
        assert np.array_equal(idx[:m], np.flatnonzero(mask)) and (idx[m:] == -7).all()
        # and without the index list
        assert same_bits(scene.select(d_keep).download(), soa[:, mask])

    # out-of-range indices in a scene gather: clamped and counted
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    idx = np.array([5, -1, n, 7, INT32_MIN, INT32_MAX], np.int64)
    g = scene.gather(dev(torch, idx.astype(np.int32)), len(idx), bad_ptr=bad)
    assert same_bits(g.download(), soa[:, np.clip(idx, 0, n - 1)]) and int(bad.item()) == 4

    # a (narrays, n) pair that is not the block's is refused
    d_idx = dev(torch, np.arange(4, dtype=np.int32))
    d_keep = torch.ones(n + 1, dtype=torch.uint8, device="cuda")
    other = {38: 49, 49: 59, 59: 38}[narrays]
    for na, nn in ((other, n), (narrays, n + 1), (narrays, n - 1)):
        wrong = gpu.Scene(scene.ptr, nn, owned=False, narrays=na)
        with pytest.raises(gpu.GsrError, match="block holds"):
            wrong.gather(d_idx, 4)
        with pytest.raises(gpu.GsrError, match="block holds"):
            wrong.select(d_keep)
    # so is memory that is no scene block (an AoS array's first floats are never the magic)
    aos = torch.zeros(4096, dtype=torch.float32, device="cuda")
    with pytest.raises(gpu.GsrError, match="not a scene block"):
        gpu.Scene(aos.data_ptr(), 8, owned=False).gather(d_idx, 4)


# ---------------------------------------------------------------- 4. prune invariance

def frame(gsr, torch, r, scene, cam, W, H, time=None):
    out = torch.full((3 * W * H,), float("nan"), dtype=torch.float32, device="cuda")
    for _ in range(3):
        r.render(scene, cam, W, H, out.data_ptr(), time=time)
        if r.sync() == 0:
            return out.view(3, H, W).cpu().numpy()
    raise AssertionError("frame still incomplete after three renders")


def count_into(gsr, torch, r, scene, cam, W, H, count, time=None):
    """One complete contrib frame accumulated into the device count buffer."""
    before = count.clone()
    for attempt in range(3):
        if attempt:
            count.copy_(before)
        r.render_contrib(scene, cam, W, H, count_ptr=count.data_ptr(), time=time)
        if r.sync() == 0:
            return
    raise AssertionError("contrib frame still incomplete after three renders")


def exact_renderer(gsr, diagnostics=False):
    r = gsr.Renderer()
    r.set_tuning(KNOB_BLEND_EXP, 0)
    if diagnostics:
        r.set_diagnostics(True)
    return r


def prune_by_count(gsr, torch, scene, count):
    """Mask count > 0 built on the device, then Scene.select: (pruned scene, host keep mask,
    device index list)."""
    d_keep = (count != 0).to(torch.uint8)
    d_idx = torch.full((scene.n,), -7, dtype=torch.int32, device="cuda")
    pruned = scene.select(d_keep, d_idx)
    keep = d_keep.cpu().numpy().astype(bool)
    assert pruned.n == int(keep.sum())
    assert np.array_equal(d_idx.cpu().numpy()[:pruned.n], np.flatnonzero(keep))
    return pruned, keep, d_idx


def prune_one_camera(gsr, orc, torch, soa, scene, ci, W, H):
    """render -> render_contrib -> select -> render for one camera, with every image and
    take-map check of the prune-invariance cases; returns (keep, visible) host masks."""
    n = soa.shape[1]
    cam = cam_for(gsr, W, H, **CAMS[ci])
    r = exact_renderer(gsr, diagnostics=True)
    full = frame(gsr, torch, r, scene, cam, W, H)
    takes_full = r.take_map(W, H) & np.uint64(0xFFFFFFFF)
    visible = r.read_splats(n)["tile_count"] > 0
    count = torch.zeros(n, dtype=torch.int32, device="cuda")
    count_into(gsr, torch, r, scene, cam, W, H, count)
    pruned, keep, _ = prune_by_count(gsr, torch, scene, count)
    print(f"camera {ci}: kept {pruned.n} of {n}, dropped {int((visible & ~keep).sum())} visible ones")
    assert int(count.cpu().numpy().view(np.uint32).astype(np.int64).sum()) == int(takes_full.sum())

    got = frame(gsr, torch, r, pruned, cam, W, H)
    assert same_bits(got, full)
    assert np.array_equal(r.take_map(W, H) & np.uint64(0xFFFFFFFF), takes_full)
    assert same_bits(got, orc.render(np.ascontiguousarray(soa[:, keep]), cam, W, H, 3.0))
    assert (full != 0).sum() > 100
    count_p = torch.zeros(pruned.n, dtype=torch.int32, device="cuda")
    count_into(gsr, torch, r, pruned, cam, W, H, count_p)
    assert np.array_equal(count_p.cpu().numpy(), count.cpu().numpy()[keep])
    return keep, visible


@pytest.mark.parametrize("ci", range(len(CAMS)))
def test_prune_invariance_occlusion(gpu, orc, torch, dense, ci):
    """600 dense Gaussians at 64 x 48: most of what goes was visible to the preprocess and is
    hidden behind saturated pixels.  Each camera must drop at least 40 such Gaussians (the
    oracle alone drops 67, 63, 165 and 58), so the test cannot pass by pruning nothing or only
    what the preprocess had culled."""
    soa, scene = dense
    keep, visible = prune_one_camera(gpu, orc, torch, soa, scene, ci, 64, 48)
    assert int((visible & ~keep).sum()) >= 40
    assert not (keep & ~visible).any()


@pytest.mark.parametrize("ci", range(len(CAMS)))
def test_prune_invariance_culling(gpu, orc, torch, c1, scene1, ci):
    """The 10,000-Gaussian synthetic scene at 333 x 217 (the oracle keeps 8,966, 9,548, 6,499
    and 8,475)."""
    keep, _ = prune_one_camera(gpu, orc, torch, c1[1], scene1, ci, 333, 217)
    assert 1000 < keep.sum() < keep.size


def test_multi_view_prune(gpu, torch, c1, scene1):
    """The count accumulated over the four cameras, one prune: every view is unchanged."""
    W, H = 333, 217
    n = scene1.n
    cams = [cam_for(gpu, W, H, **c) for c in CAMS]
    r = exact_renderer(gpu)
    full = [frame(gpu, torch, r, scene1, cam, W, H) for cam in cams]
    count = torch.zeros(n, dtype=torch.int32, device="cuda")
    for cam in cams:
        count_into(gpu, torch, r, scene1, cam, W, H, count)
    pruned, keep, _ = prune_by_count(gpu, torch, scene1, count)
    print("multi-view: kept", pruned.n, "of", n)
    assert 1000 < pruned.n < n
    for cam, want in zip(cams, full):
        assert (want != 0).sum() > 1000
        assert same_bits(frame(gpu, torch, r, pruned, cam, W, H), want)


def test_prune_4d_and_sh3(gpu, torch, tmp_path_factory, c1):
    """A 4D scene at a fixed time and an SH-3 scene: the pruned render equals the full render
    bit for bit (both from the GPU's exact blend)."""
    W, H = 320, 200
    p = tmp_path_factory.mktemp("ops4d") / "scene4d.ply"
    gpu.write_synthetic_ply4d(str(p), 4_000, 5)
    s4d = gpu.Scene.from_soa(gpu.read_ply(str(p), four_d=True))
    sh3 = gpu.Scene.from_ply(c1[0], sh3=True)
    assert s4d.is_4d and sh3.is_sh3
    for scene, time in ((s4d, 0.3), (sh3, None)):
        cam = cam_for(gpu, W, H, **CAMS[1])
        r = exact_renderer(gpu)
        full = frame(gpu, torch, r, scene, cam, W, H, time=time)
        count = torch.zeros(scene.n, dtype=torch.int32, device="cuda")
        count_into(gpu, torch, r, scene, cam, W, H, count, time=time)
        pruned, keep, _ = prune_by_count(gpu, torch, scene, count)
        print("4D" if scene.is_4d else "SH-3", "kept", pruned.n, "of", scene.n)
        assert 100 < pruned.n < scene.n and pruned.narrays == scene.narrays
        assert (full != 0).sum() > 1000
        assert same_bits(frame(gpu, torch, r, pruned, cam, W, H, time=time), full)


# ---------------------------------------------------------------- 5. side arrays follow the scene

def test_feature_planes_follow_the_scene(gpu, orc, torch, c1, scene1):
    """render_aux with two oracle-coloured feature planes (tests/test_gpu_aux.py) on the full
    scene, and on the pruned scene with the features compacted by gather_planes through the
    index list select() returned: the composited feature planes are equal bit for bit."""
    W, H, ci = 333, 217, 1
    soa = c1[1]
    n = soa.shape[1]
    cam = cam_for(gpu, W, H, **CAMS[ci])
    feat = np.ascontiguousarray(orc.preprocess(random_soa(soa), cam, W, H, 3.0)["color"].T[:2])
    assert feat.shape == (2, n)
    d_feat = dev(torch, feat)
    r = exact_renderer(gpu)

    def feat_planes(scene, d_features):
        out = torch.full((2, H, W), float("nan"), dtype=torch.float32, device="cuda")
        for _ in range(3):
            r.render_aux(scene, cam, W, H, features_ptr=d_features.data_ptr(), nfeat=2, feat_out_ptr=out.data_ptr())
            if r.sync() == 0:
                return out.cpu().numpy()
        raise AssertionError("aux frame still incomplete after three renders")

    want = feat_planes(scene1, d_feat)
    assert (want != 0).sum() > 1000
    count = torch.zeros(n, dtype=torch.int32, device="cuda")
    count_into(gpu, torch, r, scene1, cam, W, H, count)
    pruned, keep, d_idx = prune_by_count(gpu, torch, scene1, count)
    m = pruned.n
    assert 1000 < m < n
    d_feat_p = torch.full((2, m), float("nan"), dtype=torch.float32, device="cuda")
    gpu.gather_planes(d_feat_p, m, d_feat, n, 2, 4, n, d_idx, m)
    assert same_bits(d_feat_p.cpu().numpy(), feat[:, keep])
    assert same_bits(feat_planes(pruned, d_feat_p), want)
    # the accumulated statistics are cut down the same way (uint32 and uint64 elements)
    weight = torch.zeros(n, dtype=torch.int64, device="cuda")
    r.render_contrib(scene1, cam, W, H, weight_ptr=weight.data_ptr())
    assert r.sync() == 0
    weight_p = torch.full((m,), -1, dtype=torch.int64, device="cuda")
    count_p = torch.full((m,), -1, dtype=torch.int32, device="cuda")
    gpu.gather_planes(weight_p, m, weight, n, 1, 8, n, d_idx, m)
    gpu.gather_planes(count_p, m, count, n, 1, 4, n, d_idx, m)
    assert np.array_equal(weight_p.cpu().numpy(), weight.cpu().numpy()[keep]) and (weight_p > 0).all()
    assert np.array_equal(count_p.cpu().numpy(), count.cpu().numpy()[keep])
