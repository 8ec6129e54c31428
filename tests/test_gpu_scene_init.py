"""Scene initialisation on the device (gsr_points_knn_dist2, gsr_scene_from_points;
points_knn_dist2, Scene.knn_dist2, Scene.from_points): the 3-NN statistic against the numpy twin
(tests/_points_ref.py) bit for bit over sizes around every boundary of the structure and over
clouds built to defeat a spatial key; the new block against the fill twin; and the way in: a block
made from points renders as a fresh upload of it and as the oracle does, and takes one step of the
training loop."""
import numpy as np
import pytest

import _points_ref as ref
from test_adam_ref import random_scene
from test_gpu_adam import ALL_LRS, zeros_like_groups
from test_gpu_parity import CAMS, cam_for
from test_gpu_scene_ops import assert_header, dev, exact_renderer, frame, same_bits

pytestmark = pytest.mark.gpu

GUARD = 64
SENT = 123.0
LEAF, FAN, CHUNK, TILE = ref.LEAF, ref.FAN, ref.BOUNDS_CHUNK, ref.SORT_TILE
BOX1 = LEAF * FAN            # points under a level-1 box (also the sort pass's tile: 4,096)
BOX2 = BOX1 * FAN            # points under a level-2 box
INF = float("inf")


@pytest.fixture(scope="module")
def torch(gpu):
    import torch as t
    assert t.cuda.is_available()
    return t


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_structure_constants(gpu):
    assert (LEAF, FAN, CHUNK, TILE) == (gpu.KNN_LEAF, gpu.KNN_FAN, gpu.KNN_BOUNDS_CHUNK, gpu.KNN_SORT_TILE)
    assert BOX1 == TILE == 4096 and BOX2 == 262144


_CASES = {}


def case(name, n):
    """(cloud, the twin's mean2, the invalid count), computed once per (name, n)."""
    key = (name, n)
    if key not in _CASES:
        seed = 1000 * sorted(ref.clouds(np.random.default_rng(0), 4)).index(name) + n
        xyz = ref.clouds(np.random.default_rng(seed), n)[name] if n else np.zeros((0, 3), np.float32)
        want, bad = ref.knn_dist2(xyz)
        for a in (xyz, want):
            a.setflags(write=False)
        _CASES[key] = (xyz, want, bad)
    return _CASES[key]


def run_knn(gsr, torch, xyz, planar, stream=None, skew=0):
    """One call with guards everywhere: (mean2 [n], bad).  planar: plane stride n + 37; skew:
    bytes the scratch pointer is moved off its 256-byte alignment."""
    n = xyz.shape[0]
    if planar:
        S = n + 37
        host = np.full((3, S), np.nan, np.float32)
        host[:, :n] = xyz.T
        strides = dict(point_stride=1, comp_stride=S)
    else:
        host = np.concatenate([xyz.reshape(-1), np.full(GUARD, np.nan, np.float32)])
        strides = dict(point_stride=3, comp_stride=1)
    d_xyz = dev(torch, host)
    d_out = torch.full((n + GUARD,), SENT, dtype=torch.float32, device="cuda")
    nbytes = gsr.points_knn_scratch_bytes(n)
    d_scratch = torch.full((skew + nbytes + 4 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    d_bad = torch.zeros(2, dtype=torch.int32, device="cuda")
    s = stream.cuda_stream if stream is not None else 0
    torch.cuda.synchronize()   # the buffers above were filled on the default stream
    gsr.points_knn_dist2(d_xyz.data_ptr(), n, d_out, d_scratch.data_ptr() + skew, nbytes, bad_ptr=d_bad, stream=s,
                         **strides)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert (out[n:] == SENT).all(), "wrote past d_mean2[n)"
    assert (d_scratch[skew + nbytes:].cpu().numpy() == 0xA5).all(), "wrote past scratch_bytes"
    assert (d_scratch[:skew].cpu().numpy() == 0xA5).all()
    assert np.array_equal(d_xyz.cpu().numpy().view(np.uint32), host.view(np.uint32)), "the input changed"
    b = d_bad.cpu().numpy()
    assert b[1] == 0
    return out[:n], int(b[0])


def check_knn(gsr, torch, xyz, want, bad, what):
    other = torch.cuda.Stream()
    got_i, bad_i = run_knn(gsr, torch, xyz, planar=False)
    got_p, bad_p = run_knn(gsr, torch, xyz, planar=True, stream=other, skew=4)
    for got, lay in ((got_i, "interleaved"), (got_p, "planar")):
        diff = np.flatnonzero(bits(got) != bits(want))
        assert diff.size == 0, f"{what} {lay}: {diff.size} differ, first {diff[:6].tolist()}: " \
                               f"{got[diff[:6]].tolist()} != {want[diff[:6]].tolist()}"
    assert bad_i == bad_p == bad, what
    return got_i


# ---------------------------------------------------------------- 1. the statistic

SIZES = [0, 1, 2, 3, 4, 5, LEAF - 1, LEAF, LEAF + 1, 1000, CHUNK - 1, CHUNK, CHUNK + 1, BOX1 - 1, BOX1, BOX1 + 1,
         12289]


@pytest.mark.parametrize("n", SIZES)
def test_knn_sizes(gpu, torch, n):
    """Around the leaf (64), the bounds kernel's chunk (2,048) and the level-1 box and sort tile
    (4,096), on the clustered cloud; the small sizes take k = 0, 1, 2."""
    xyz, want, bad = case("clustered", n)
    check_knn(gpu, torch, xyz, want, bad, f"clustered n={n}")
    if 0 < n <= 5:
        for name in ("huge", "identical", "nonfinite"):
            check_knn(gpu, torch, *case(name, n), f"{name} n={n}")


@pytest.mark.parametrize("n", [BOX2 - 1, BOX2, BOX2 + 1])
def test_knn_level2_boundary(gpu, torch, n):
    """Around the level-2 box (262,144 points).  The twin is O(n) per row, so 256 rows are
    compared: the first and last leaves and a random sample; the two runs are compared in full."""
    rng = np.random.default_rng(n)
    xyz = ref.clustered(rng, n, clusters=200)
    rows = np.unique(np.concatenate([np.arange(32), np.arange(n - 32, n), rng.choice(n, 192, replace=False)]))
    want = ref.knn_rows(xyz, rows, chunk=32)
    a, bad_a = run_knn(gpu, torch, xyz, planar=False)
    b, bad_b = run_knn(gpu, torch, xyz, planar=True, stream=torch.cuda.Stream(), skew=8)
    assert np.array_equal(bits(a[rows]), bits(want)), np.flatnonzero(bits(a[rows]) != bits(want))[:8]
    assert np.array_equal(bits(a), bits(b)) and bad_a == bad_b == 0


CLOUDS = ["uniform", "clustered", "plane", "line", "identical", "duplicated", "lattice", "two_far_clusters",
          "outliers", "huge", "offset", "nonfinite"]


@pytest.mark.parametrize("n", [LEAF + 1, 1000, BOX1 + 1])
@pytest.mark.parametrize("name", CLOUDS)
def test_knn_clouds(gpu, torch, name, n):
    xyz, want, bad = case(name, n)
    got = check_knn(gpu, torch, xyz, want, bad, f"{name} n={n}")
    ok = ref.valid_mask(xyz)
    if name == "nonfinite":
        assert bad == max(3, n // 100) and not bits(got[~ok]).any()
        # the bad points influence nobody: the valid points alone give the same values
        alone, _ = ref.knn_dist2(xyz[ok])
        assert np.array_equal(bits(got[ok]), bits(alone))
    else:
        assert bad == 0
    if name == "identical":
        assert not bits(got).any()                      # every distance 0, every key equal
    if name == "huge" and n <= 1000:
        assert np.isinf(case(name, 4)[1]).any()        # d2 overflows at the smallest size
    if name == "lattice":
        assert (got == 1.0).sum() > n // 4              # massive exact ties


# ---------------------------------------------------------------- 2. on a block's own planes

def test_scene_knn_dist2(gpu, torch):
    n = 1000
    soa = random_scene(38, n, np.random.default_rng(4)).astype(np.float32)
    scene = gpu.Scene.from_soa(soa)
    xyz = np.ascontiguousarray(scene.download()[0:3].T)
    nbytes = gpu.points_knn_scratch_bytes(n)
    d_scratch = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    d_out = torch.full((n + GUARD,), SENT, dtype=torch.float32, device="cuda")
    scene.knn_dist2(d_out, d_scratch, nbytes)
    d_out2 = torch.full((n,), SENT, dtype=torch.float32, device="cuda")
    gpu.points_knn_dist2(dev(torch, xyz), n, d_out2, d_scratch, nbytes)
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    assert (got[n:] == SENT).all()
    assert np.array_equal(bits(got[:n]), bits(d_out2.cpu().numpy()))
    assert np.array_equal(bits(got[:n]), bits(ref.knn_dist2(xyz)[0]))
    assert same_bits(scene.download(), soa)


# ---------------------------------------------------------------- 3. the initialiser

@pytest.mark.parametrize("narrays", [38, 49, 59])
def test_from_points(gpu, torch, narrays):
    n = 1000
    xyz, mean2, bad = case("nonfinite", n)
    rng = np.random.default_rng(narrays)
    rgb = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    rgb[0] = [0.5, np.nan, np.inf]                          # non-finite colours propagate
    d_xyz, d_rgb = dev(torch, xyz.copy()), dev(torch, rgb)
    d_mean2 = torch.full((n + GUARD,), SENT, dtype=torch.float32, device="cuda")
    d_bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    cfg = dict(t_center=0.25, t_scale=0.5) if narrays == 49 else {}

    scene = gpu.Scene.from_points(d_xyz, n, d_rgb, narrays=narrays, mean2_ptr=d_mean2, bad_ptr=d_bad, **cfg)
    assert_header(gpu, torch, scene, narrays, n)
    got = scene.download()
    want = ref.fill(xyz, rgb, mean2, narrays, **cfg)
    diff = bits(got) != bits(want)
    assert got.shape == want.shape and not diff.any(), f"(array, j) {np.argwhere(diff)[:8].tolist()}"
    m2 = d_mean2.cpu().numpy()
    assert np.array_equal(bits(m2[:n]), bits(mean2)) and (m2[n:] == SENT).all() and int(d_bad.item()) == bad == 10
    # invalid points: the position's bits, the floor scale
    ok = ref.valid_mask(xyz)
    assert np.array_equal(bits(got[0:3][:, ~ok]), bits(xyz[~ok].T)) and not np.isfinite(got[0:3][:, ~ok]).all(axis=0).any()
    assert (got[4:7][:, ~ok] == np.sqrt(np.float32(1e-7))).all()
    assert np.isnan(got[12, 0]) and np.isinf(got[13, 0]) and got[11, 0] == 0

    # no colours, no outputs; a factor and a cap that bites on some
    cap = float(np.median(np.sqrt(np.maximum(mean2, np.float32(1e-9))) * np.float32(2.0)))
    opts = dict(opacity=0.3, min_dist2=1e-9, scale_mul=2.0, scale_max=cap)
    grey = gpu.Scene.from_points(d_xyz, n, None, narrays=narrays, **opts, **cfg)
    assert_header(gpu, torch, grey, narrays, n)
    g = grey.download()
    assert same_bits(g, ref.fill(xyz, None, mean2, narrays, **opts, **cfg))
    assert not bits(g[11:14]).any() and (g[3] == np.float32(0.3)).all()
    assert (g[4] == np.float32(cap)).sum() > n // 4 and (g[4] < np.float32(cap)).sum() > n // 4

    # planar points and colours (a block's own layout), the same block
    S = n + 24
    pl, cl = np.zeros((3, S), np.float32), np.zeros((3, S), np.float32)
    pl[:, :n], cl[:, :n] = xyz.T, rgb.T
    planar = gpu.Scene.from_points(dev(torch, pl), n, dev(torch, cl), narrays=narrays, point_stride=1, comp_stride=S,
                                   rgb_point_stride=1, rgb_comp_stride=S, **cfg)
    assert same_bits(planar.download(), want)


def test_from_no_points(gpu, torch):
    for narrays in (38, 49, 59):
        empty = gpu.Scene.from_points(None, 0, narrays=narrays)
        assert_header(gpu, torch, empty, narrays, 0)
        assert empty.download().shape == (narrays, 0)


# ---------------------------------------------------------------- 4. the way in

W = H = 64


def test_points_to_training_step(gpu, orc, torch):
    """400 coloured points at 64 x 64: the block from_points builds renders through one
    exact-blend context exactly as a fresh upload of its download and as the oracle renders that
    download; then one pass of image_loss -> render_backward_scene -> adam_step -> densify with
    finite gradients.  No claim about the loss value is tested."""
    n = 400
    rng = np.random.default_rng(31)
    xyz = rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32)
    rgb = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    scene = gpu.Scene.from_points(dev(torch, xyz), n, dev(torch, rgb), opacity=0.5, scale_mul=1.0)
    assert_header(gpu, torch, scene, 38, n)
    soa = scene.download()
    assert same_bits(soa, ref.fill(xyz, rgb, ref.knn_dist2(xyz)[0], 38, opacity=0.5))
    cam = cam_for(gpu, W, H, **CAMS[0])
    r = exact_renderer(gpu, diagnostics=True)
    got = frame(gpu, torch, r, scene, cam, W, H)
    takes = r.take_map(W, H)
    r2 = exact_renderer(gpu, diagnostics=True)
    fresh = frame(gpu, torch, r2, gpu.Scene.from_soa(soa), cam, W, H)
    assert same_bits(got, fresh) and np.array_equal(takes, r2.take_map(W, H))
    assert same_bits(got, orc.render(soa, cam, W, H, 3.0))
    assert (got != 0).sum() > 1000

    target = dev(torch, rng.uniform(0, 1, 3 * W * H).astype(np.float32))
    image = torch.zeros(3 * W * H, dtype=torch.float32, device="cuda")
    grad_image = torch.zeros_like(image)
    scratch_bytes = gpu.image_loss_scratch_bytes(W, H, True)
    loss_scratch = torch.zeros(scratch_bytes // 4, dtype=torch.float32, device="cuda")
    record = torch.zeros(10 * n, dtype=torch.float32, device="cuda")
    g, m, v = (zeros_like_groups(torch, n) for _ in range(3))
    d_accum = torch.zeros(n, dtype=torch.float32, device="cuda")
    d_seen = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    for attempt in range(3):
        r.render(scene, cam, W, H, image.data_ptr())
        gpu.image_loss(image, target, W, H, grad_ptr=grad_image, scratch_ptr=loss_scratch, scratch_bytes=scratch_bytes)
        for t in g.values():
            t.zero_()
        r.render_backward_scene(scene, cam, W, H, grad_image_ptr=grad_image, scratch_ptr=record,
                                **{k + "_ptr": t for k, t in g.items()})
        if r.sync() == 0:
            break
    else:
        raise AssertionError("frame still incomplete after three renders")
    for k, t in g.items():
        h = t.cpu().numpy()
        assert np.isfinite(h).all(), k
    assert any(t.cpu().numpy().any() for t in g.values())
    gpu.densify_accumulate(record[8 * n:], n, W, H, d_accum, d_seen, bad_ptr=d_bad)
    scene.adam_step(g, m, v, step=1, bad_ptr=d_bad, **ALL_LRS)
    grown, rep = scene.densify(d_accum, d_seen, grad_threshold=0.0, scale_split=float(np.median(soa[4])),
                               min_opacity=0.005, seed=3)
    torch.cuda.synchronize()
    assert int(d_bad.item()) == 0
    assert rep["kept"] + rep["cloned"] + rep["split"] + rep["pruned"] == n and grown.n == rep["n_out"] > n
    assert np.isfinite(grown.download()).all()
