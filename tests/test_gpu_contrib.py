"""Contribution statistics (gsr_render_contrib, Renderer.render_contrib): per-Gaussian
count / fixed-point weight / max weight and the per-pixel id plane, against the UNMODIFIED
CPU oracle, exactly.

The oracle only renders colours, but its colour is clamp(C0 f_dc + 0.5, 0, 1) per channel
with f_rest (SoA arrays 14..37) zeroed: f_dc = -4 gives exactly 0.0 and f_dc = +4 exactly
1.0.  In a copy of the scene where every f_dc is -4 except f_dc[ch, i] = +4 for one
Gaussian i per channel, channel ch of the oracle's image is exactly the plane
w_i(p) = fma(alpha, T, 0) of Gaussian i (fma(0 alpha, T, acc) = acc for the others): one
oracle render gives three Gaussians' weight planes over the unchanged geometry.  From a
plane: count = its non-zero pixels, max = its maximum, weight = sum of rint(w 2^24)."""
import numpy as np
import pytest

from conftest import assert_frames, scene_soa
from test_gpu_parity import CAMS, cam_for

pytestmark = pytest.mark.gpu

F_DC, F_REST = slice(11, 14), slice(14, 38)
ID_SENTINEL = -7
MIX = 2654435761
KNOB_BLEND_EXP, KNOB_SPLIT, KNOB_PM, KNOB_STATE = 22, 23, 24, 26


@pytest.fixture(scope="module")
def torch(gpu):
    import torch as t
    assert t.cuda.is_available()
    return t


@pytest.fixture(scope="module")
def c1(gpu, tmp_path_factory):
    return scene_soa(gpu, tmp_path_factory, 10_000, 1)[1]


@pytest.fixture(scope="module")
def scene1(gpu, c1):
    return gpu.Scene.from_soa(c1)


def dense_soa():
    rng = np.random.default_rng(22); n = 200
    soa = np.zeros((38, n), np.float32)
    soa[0:3] = rng.uniform(-0.5, 0.5, (3, n)); soa[3] = rng.uniform(0.5, 0.99, n)
    soa[4:7] = rng.uniform(0.1, 0.4, (3, n)); soa[7] = 1.0
    soa[11:38] = rng.normal(0, 0.3, (27, n))
    return soa


@pytest.fixture(scope="module")
def dense(gpu):
    soa = dense_soa()
    return soa, gpu.Scene.from_soa(soa)


@pytest.fixture(scope="module")
def tilted(gpu):
    """_wide_scenes' tilted scene: random quaternions (the dense scene's is the identity), so
    the conics carry off-diagonal terms of their own and the ellipses cross blocks at an angle."""
    from _wide_scenes import scene as wide_scene
    soa = wide_scene("tilted")
    return soa, gpu.Scene.from_soa(soa)


# ---------------------------------------------------------------- the reference

def marked_soa(soa, ids):
    """Up to three Gaussians, one per colour channel, coloured exactly 1.0; all others 0.0."""
    s = soa.copy()
    s[F_REST] = 0.0
    s[F_DC] = -4.0
    for ch, i in enumerate(ids):
        s[11 + ch, i] = 4.0
    return s


def ones_soa(soa):
    s = soa.copy()
    s[F_REST] = 0.0
    s[11] = 4.0
    return s


def weight_planes(orc, soa, cam, W, H, ids, tiling=None):
    """{i: the (H, W) plane w_i(p)} for the Gaussians `ids`, three per oracle render."""
    ids = [int(i) for i in ids]
    out = {}
    for j in range(0, len(ids), 3):
        g = ids[j:j + 3]
        img = orc.render(marked_soa(soa, g), cam, W, H, 3.0, tiling=tiling)
        for ch, i in enumerate(g):
            out[i] = img[ch].copy()
    return out


def plane_stats(w):
    """(count, weight, max bits) of one weight plane, as gsr_render_contrib defines them."""
    assert (w >= 0).all() and float(w.max(initial=0.0)) <= 0.99
    count = int((w != 0).sum())
    weight = int(np.rint(w * np.float32(16777216)).astype(np.uint64).sum())
    mx = int(np.float32(w.max(initial=0.0)).view(np.uint32))
    return count, weight, mx


_dense_refs = {}


def dense_ref(orc, gsr, soa, W, H, tiling=None, name="dense"):
    """All 200 planes of the dense (or tilted) scene (67 oracle renders), once per (scene, size,
    tiling): {"P": (n, H, W), "count", "weight", "max": (n,), "id": (H, W)}."""
    key = (name, W, H, tiling)
    if key not in _dense_refs:
        n = soa.shape[1]
        cam = cam_for(gsr, W, H)
        pl = weight_planes(orc, soa, cam, W, H, range(n), tiling)
        P = np.stack([pl[i] for i in range(n)])
        st = [plane_stats(P[i]) for i in range(n)]
        ident = np.where((P != 0).any(0), P.argmax(0), -1).astype(np.int32)
        ref = {"P": P, "count": np.array([s[0] for s in st], np.uint32),
               "weight": np.array([s[1] for s in st], np.uint64), "max": np.array([s[2] for s in st], np.uint32),
               "id": ident}
        for v in ref.values():
            v.setflags(write=False)
        _dense_refs[key] = ref
    return _dense_refs[key]


# ---------------------------------------------------------------- the GPU side

def tiling_of(gsr, W, H, tiling):
    if tiling is None:
        return None
    t = gsr.TilingInformation(1, 1, H, W)
    t.num_tile_x, t.num_tile_y, t.width_stride, t.height_stride = tiling
    return t


def new_bufs(torch, n, W, H, what="cwmi", fill=(0, 0, 0)):
    """Device buffers of the outputs in `what` (c count, w weight, m max, i id); the id plane
    starts as a sentinel, so a pixel the frame leaves unwritten fails any comparison."""
    b = {}
    if "c" in what:
        b["count"] = torch.full((n,), fill[0], dtype=torch.int32, device="cuda")
    if "w" in what:
        b["weight"] = torch.full((n,), fill[1], dtype=torch.int64, device="cuda")
    if "m" in what:
        b["max"] = torch.full((n,), fill[2], dtype=torch.int32, device="cuda")
    if "i" in what:
        b["id"] = torch.full((H, W), ID_SENTINEL, dtype=torch.int32, device="cuda")
    return b


def to_host(b):
    views = {"count": np.uint32, "weight": np.uint64, "max": np.uint32, "id": np.int32}
    return {k: v.cpu().numpy().view(views[k]) for k, v in b.items()}


def contrib_into(gsr, torch, r, scene, cam, W, H, b, tiling=None, n=None, time=None):
    """One complete contrib frame into the buffers b (accumulating): up to three renders until
    sync() == 0, the buffers put back to their state before the frame ahead of each retry."""
    before = {k: v.clone() for k, v in b.items()}
    ptr = lambda k: b[k].data_ptr() if k in b else None   # noqa: E731
    for attempt in range(3):
        if attempt:
            for k, v in b.items():
                v.copy_(before[k])
        r.render_contrib(scene, cam, W, H, count_ptr=ptr("count"), weight_ptr=ptr("weight"), max_ptr=ptr("max"),
                         id_ptr=ptr("id"), tiling=tiling_of(gsr, W, H, tiling), n=n, time=time)
        if r.sync() == 0:
            return
    raise AssertionError("contrib frame still incomplete after three renders")


def contrib(gsr, torch, scene, cam, W, H, what="cwmi", tiling=None, renderer=None, n=None, time=None):
    """One contrib frame into freshly zeroed buffers; returns the requested arrays on the host."""
    r = renderer or gsr.Renderer()
    b = new_bufs(torch, scene.n, W, H, what)
    contrib_into(gsr, torch, r, scene, cam, W, H, b, tiling=tiling, n=n, time=time)
    return to_host(b)


def plain(gsr, torch, scene, cam, W, H, renderer):
    out = torch.empty(3 * W * H, dtype=torch.float32, device="cuda")
    for _ in range(3):
        renderer.render(scene, cam, W, H, out.data_ptr())
        if renderer.sync() == 0:
            break
    return out.view(3, H, W).cpu().numpy()


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def assert_contrib_equal(got, ref, keys=("count", "weight", "max", "id")):
    for k in keys:
        assert got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), \
            (k, np.flatnonzero((got[k] != ref[k]).ravel())[:8])


# ---------------------------------------------------------------- 1. dense scene, every Gaussian

@pytest.mark.parametrize("name,W,H", [("dense", 96, 64), ("tilted", 128, 80)])
def test_dense_scene_every_gaussian_exact(gpu, orc, torch, request, name, W, H):
    """96 x 64, 200 Gaussians (and the tilted scene's 200 at 128 x 80): all four outputs equal
    the oracle's planes exactly.  The reference is first shown to hold what makes the
    comparison meaningful: lists longer than one batch and no ties; for the dense scene also
    saturated pixels and dominant splats that are not the nearest."""
    soa, scene = request.getfixturevalue(name)
    cam = cam_for(gpu, W, H)
    ref = dense_ref(orc, gpu, soa, W, H, name=name)
    P = ref["P"]
    takes = (P != 0).sum(0)
    print("max takes per pixel", int(takes.max()))
    assert takes.max() > 64
    ties = ((P == P.max(0)) & (P.max(0) > 0)).sum(0) > 1
    print("ties", int(ties.sum()))
    assert ties.sum() == 0
    spl = orc.preprocess(soa, cam, W, H, 3.0)
    if name == "dense":     # what this scene was built for
        alpha = orc.render(ones_soa(soa), cam, W, H, 3.0)[0]
        print("saturated pixels", int((alpha >= 0.999).sum()))
        assert (alpha >= 0.999).sum() >= 500
        order = (orc.expected_depth_order(spl) & np.uint64(0xFFFFFFFF)).astype(np.int64)
        nearest = order[(P[order] != 0).argmax(0)]
        dom_not_near = (takes > 0) & (ref["id"] != nearest)
        print("dominant != nearest", int(dom_not_near.sum()))
        assert dom_not_near.sum() >= 1000
    hidden = (spl["status"] == 2) & (ref["count"] == 0)
    print("visible but never composited", int(hidden.sum()))
    # the take map agrees with the planes (count and index hash per pixel)
    tk = orc.render_takes(soa, cam, W, H, 3.0)[1]
    assert np.array_equal(tk & np.uint64(0xFFFFFFFF), takes.astype(np.uint64))

    got = contrib(gpu, torch, scene, cam, W, H)
    assert_contrib_equal(got, ref)


@pytest.mark.parametrize("W,H", [(37, 23), (1, 1)])
def test_dense_scene_odd_sizes(gpu, orc, torch, dense, W, H):
    soa, scene = dense
    got = contrib(gpu, torch, scene, cam_for(gpu, W, H), W, H)
    assert_contrib_equal(got, dense_ref(orc, gpu, soa, W, H))


def test_dense_scene_partial_tiling(gpu, orc, torch, dense):
    """Tiling (3, 2, 20, 20) covers 60 x 40 of 96 x 64: the statistics are the covered
    area's, and d_id is -1 outside it."""
    soa, scene = dense
    W, H, tiling = 96, 64, (3, 2, 20, 20)
    ref = dense_ref(orc, gpu, soa, W, H, tiling)
    assert not ref["P"][:, 40:, :].any() and not ref["P"][:, :, 60:].any() and ref["count"].sum() > 1000
    got = contrib(gpu, torch, scene, cam_for(gpu, W, H), W, H, tiling=tiling)
    assert (got["id"][40:, :] == -1).all() and (got["id"][:, 60:] == -1).all()
    assert_contrib_equal(got, ref)


@pytest.mark.parametrize("knobs", [{13: 0}, {7: 0}, {28: 0}])
def test_knobs_do_not_change_contrib_outputs(gpu, orc, torch, dense, knobs):
    """Block mapping (13), the pair-sort path (7 = 0) and the LSD depth sort (28 = 0)."""
    soa, scene = dense
    W, H = 96, 64
    ref = dense_ref(orc, gpu, soa, W, H)
    r = gpu.Renderer()
    for kn, v in knobs.items():
        r.set_tuning(kn, v)
    for _ in range(2):   # the second frame of a context takes the bucket sort (28)
        assert_contrib_equal(contrib(gpu, torch, scene, cam_for(gpu, W, H), W, H, renderer=r), ref)


# ---------------------------------------------------------------- 2. 10,000 Gaussians

@pytest.mark.parametrize("W,H", [(333, 217), (640, 480)])
def test_synthetic_scene_identities_and_samples(gpu, orc, torch, c1, scene1, W, H):
    """Global identities against the oracle's take map, and exact statistics of 24 sampled
    Gaussians (the 12 nearest, 6 around the median, 6 farthest visible ones)."""
    n = c1.shape[1]
    cam = cam_for(gpu, W, H, **CAMS[1])
    got = contrib(gpu, torch, scene1, cam, W, H)
    tk = orc.render_takes(c1, cam, W, H, 3.0)[1]
    tcount = (tk & np.uint64(0xFFFFFFFF)).astype(np.int64)
    cnt = got["count"].astype(np.int64)
    print("take total", int(tcount.sum()))
    if (W, H) == (333, 217):
        assert tcount.sum() == 90_577
    assert cnt.sum() == tcount.sum()
    # (no overflow: counts < 2^19, mixes < 2^32, 10^4 terms; 2^19 hashes < 2^32)
    mix = (np.arange(1, n + 1, dtype=np.uint64) * np.uint64(MIX)) % np.uint64(2 ** 32)
    assert int((got["count"].astype(np.uint64) * mix).sum()) % 2 ** 32 == int((tk >> np.uint64(32)).sum()) % 2 ** 32
    spl = orc.preprocess(c1, cam, W, H, 3.0)
    assert (cnt[spl["status"] != 2] == 0).all()
    assert np.array_equal(got["id"] == -1, tcount == 0)
    assert ((got["id"] >= -1) & (got["id"] < n)).all()
    assert np.array_equal(got["max"] != 0, cnt != 0) and np.array_equal(got["weight"] != 0, cnt != 0)

    order = orc.expected_depth_order(spl)
    vis = (order[:int((spl["status"] == 2).sum())] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert (spl["status"][vis] == 2).all() and len(vis) > 100
    mid = len(vis) // 2
    sample = list(vis[:12]) + list(vis[mid - 3:mid + 3]) + list(vis[-6:])
    assert len(set(sample)) == 24
    planes = weight_planes(orc, c1, cam, W, H, sample)
    ref_counts = []
    for i in sample:
        c, w, m = plane_stats(planes[i])
        ref_counts.append(c)
        assert (int(got["count"][i]), int(got["weight"][i]), int(got["max"][i])) == (c, w, m), i
        assert (planes[i][got["id"] == i] > 0).all(), i
    print("sampled reference counts", min(ref_counts), "..", max(ref_counts))
    assert max(ref_counts) > 0


# ---------------------------------------------------------------- 3. accumulation

def test_accumulation_over_two_cameras(gpu, torch, c1, scene1):
    """Buffers zeroed once, two cameras: count and weight add, max is the element-wise
    maximum, d_id is the second frame's; each output alone equals the all-outputs call;
    two runs give identical bytes."""
    W, H = 333, 217
    n = c1.shape[1]
    cams = [cam_for(gpu, W, H, **CAMS[0]), cam_for(gpu, W, H, **CAMS[3])]
    r = gpu.Renderer()
    single = [contrib(gpu, torch, scene1, cam, W, H, renderer=r) for cam in cams]
    assert all(s["count"].sum() > 1000 for s in single)
    assert (single[0]["count"] != single[1]["count"]).any()

    def both():
        b = new_bufs(torch, n, W, H)
        for cam in cams:
            contrib_into(gpu, torch, r, scene1, cam, W, H, b)
        return to_host(b)

    acc = both()
    assert np.array_equal(acc["count"], single[0]["count"] + single[1]["count"])
    assert np.array_equal(acc["weight"], single[0]["weight"] + single[1]["weight"])
    assert np.array_equal(acc["max"], np.maximum(single[0]["max"], single[1]["max"]))
    assert np.array_equal(acc["id"], single[1]["id"])
    again = both()
    for k in acc:
        assert acc[k].tobytes() == again[k].tobytes(), k
    for what, key in (("c", "count"), ("w", "weight"), ("m", "max"), ("i", "id")):
        alone = contrib(gpu, torch, scene1, cams[1], W, H, what=what, renderer=r)
        assert set(alone) == {key} and np.array_equal(alone[key], single[1][key]), key


# ---------------------------------------------------------------- 4. pruning end to end

def exact_image(gsr, torch, soa, cam, W, H):
    r = gsr.Renderer()
    r.set_tuning(KNOB_BLEND_EXP, 0)
    return plain(gsr, torch, gsr.Scene.from_soa(soa), cam, W, H, r)


def test_pruning_by_count_keeps_the_image(gpu, orc, torch, c1, scene1, dense):
    """Gaussians no pixel composited can be dropped: the pruned scene's exact image is the
    full scene's, and the oracle's, bit for bit."""
    W, H = 333, 217
    cam = cam_for(gpu, W, H, **CAMS[2])
    keep = contrib(gpu, torch, scene1, cam, W, H, what="c")["count"] > 0
    print("pruned", int((~keep).sum()), "of", keep.size)
    assert (~keep).sum() >= 3000 and keep.sum() > 1000
    want = orc.render(c1, cam, W, H, 3.0)
    assert same_bits(exact_image(gpu, torch, np.ascontiguousarray(c1[:, keep]), cam, W, H), want)
    assert same_bits(exact_image(gpu, torch, c1, cam, W, H), want)

    soa, scene = dense
    W, H = 96, 64
    cam = cam_for(gpu, W, H)
    keep = contrib(gpu, torch, scene, cam, W, H, what="c")["count"] > 0
    spl = orc.preprocess(soa, cam, W, H, 3.0)
    assert np.array_equal(keep, dense_ref(orc, gpu, soa, W, H)["count"] > 0)
    assert ((spl["status"] == 2) & ~keep).sum() == 5     # visible, yet never composited: they go too
    want = orc.render(soa, cam, W, H, 3.0)
    assert same_bits(exact_image(gpu, torch, np.ascontiguousarray(soa[:, keep]), cam, W, H), want)


# ---------------------------------------------------------------- 5. frame policy

def test_depth_split_controller_untouched(gpu, orc, torch, c1, scene1):
    """With the depth split forced on, a contrib frame still runs one exact phase (its outputs
    are a split-free context's) and leaves the split point and the last frame's split state
    as they were; plain frames before and after it match the oracle."""
    W, H, ci = 640, 480, 0
    cam = cam_for(gpu, W, H, **CAMS[ci])
    want, tk = orc.render_takes(c1, cam, W, H, 3.0)
    tcount = tk & np.uint64(0xFFFFFFFF)
    r = gpu.Renderer()
    r.set_tuning(KNOB_SPLIT, 1)
    r.set_tuning(KNOB_PM, 150)
    for _ in range(2):   # the second split frame runs in key mode
        assert_frames(plain(gpu, torch, scene1, cam, W, H, r), want)
    assert r.sync() == 0
    pm, state = r.get_tuning(KNOB_PM), r.get_tuning(KNOB_STATE)
    assert state != 0
    got = contrib(gpu, torch, scene1, cam, W, H, renderer=r)
    assert_contrib_equal(got, contrib(gpu, torch, scene1, cam, W, H))
    assert got["count"].astype(np.int64).sum() == int(tcount.sum()) > 1000
    assert np.array_equal(got["id"] == -1, tcount == 0)
    assert (r.get_tuning(KNOB_PM), r.get_tuning(KNOB_STATE)) == (pm, state)
    assert_frames(plain(gpu, torch, scene1, cam, W, H, r), want)
    assert r.get_tuning(KNOB_STATE) != 0


def test_diagnostics_take_map_survives_a_contrib_frame(gpu, orc, torch, c1, scene1):
    """Contrib frames write no diagnostics: the take map of the preceding diagnostics frame
    (camera 0) is unchanged by a contrib frame of another camera."""
    W, H = 333, 217
    cam = cam_for(gpu, W, H, **CAMS[0])
    tk = orc.render_takes(c1, cam, W, H, 3.0)[1]
    r = gpu.Renderer()
    r.set_diagnostics(True)
    plain(gpu, torch, scene1, cam, W, H, r)
    assert np.array_equal(r.take_map(W, H), tk)
    got = contrib(gpu, torch, scene1, cam_for(gpu, W, H, **CAMS[1]), W, H, renderer=r)
    assert got["count"].sum() > 1000
    assert np.array_equal(r.take_map(W, H), tk)


def test_contrib_first_frame_with_split_on(gpu, orc, torch, c1, scene1):
    """Knobs 23 = 1 and 24 = 150 on a fresh context: the contrib frame's outputs are the
    one-phase ones, the knobs read back unchanged, a plain render() afterwards matches."""
    W, H, ci = 640, 480, 1
    cam = cam_for(gpu, W, H, **CAMS[ci])
    r = gpu.Renderer()
    r.set_tuning(KNOB_SPLIT, 1)
    r.set_tuning(KNOB_PM, 150)
    before = (r.get_tuning(KNOB_PM), r.get_tuning(KNOB_STATE))
    got = contrib(gpu, torch, scene1, cam, W, H, renderer=r)
    ref = contrib(gpu, torch, scene1, cam, W, H)           # a context with the split at its default
    assert_contrib_equal(got, ref)
    tk = orc.render_takes(c1, cam, W, H, 3.0)[1]
    assert got["count"].astype(np.int64).sum() == int((tk & np.uint64(0xFFFFFFFF)).sum())
    assert (r.get_tuning(KNOB_PM), r.get_tuning(KNOB_STATE)) == before == (150, 0)
    assert_frames(plain(gpu, torch, scene1, cam, W, H, r), orc.render(c1, cam, W, H, 3.0))


# ---------------------------------------------------------------- 6. overflow adds nothing

def test_overflow_frame_adds_nothing(gpu, orc, torch):
    """Huge splats (tests/test_gpu_aux.py's overflow scene): the first frame overflows the pair
    buffer and must leave the pre-filled accumulators exactly as they were; the re-render is
    complete and adds the oracle's numbers."""
    n = 3000
    rng = np.random.default_rng(9)
    soa = np.zeros((38, n), np.float32)
    soa[0] = rng.uniform(-0.2, 0.2, n); soa[1] = rng.uniform(-0.2, 0.2, n); soa[2] = rng.uniform(-0.2, 0.2, n)
    soa[3] = rng.uniform(0.01, 0.05, n)
    soa[4:7] = rng.uniform(1.0, 2.0, (3, n))
    soa[7] = 1.0
    soa[11:38] = rng.normal(0, 0.3, (27, n))
    W, H = 640, 480
    cam = cam_for(gpu, W, H)
    r = gpu.Renderer()
    r.reserve(n, 1024)
    scene = gpu.Scene.from_soa(soa)
    b = new_bufs(torch, n, W, H, fill=(7, 7, 0))
    ptrs = dict(count_ptr=b["count"].data_ptr(), weight_ptr=b["weight"].data_ptr(), max_ptr=b["max"].data_ptr(),
                id_ptr=b["id"].data_ptr())
    r.render_contrib(scene, cam, W, H, **ptrs)
    assert r.sync() == -5                      # overflow reported and buffer grown
    h = to_host(b)
    assert (h["count"] == 7).all() and (h["weight"] == 7).all() and (h["max"] == 0).all()
    r.render_contrib(scene, cam, W, H, **ptrs)
    assert r.sync() == 0
    assert r.pair_count() > 1_000_000
    h = to_host(b)
    tk = orc.render_takes(soa, cam, W, H, 3.0)[1]
    total = int((tk & np.uint64(0xFFFFFFFF)).sum())
    assert total > 100_000
    assert int((h["count"].astype(np.int64) - 7).sum()) == total
    assert np.array_equal(h["id"] == -1, (tk & np.uint64(0xFFFFFFFF)) == 0)
    spl = orc.preprocess(soa, cam, W, H, 3.0)
    vis = orc.expected_depth_order(spl)[:int((spl["status"] == 2).sum())] & np.uint64(0xFFFFFFFF)
    marked = [int(vis[0]), int(vis[len(vis) // 2]), int(vis[-1])]   # nearest, median, farthest
    for i, w in weight_planes(orc, soa, cam, W, H, marked).items():
        c, wt, m = plane_stats(w)
        assert (int(h["count"][i]) - 7, int(h["weight"][i]) - 7, int(h["max"][i])) == (c, wt, m), i


# ---------------------------------------------------------------- 7. edge cases

def test_empty_and_all_culled(gpu, torch, c1, scene1):
    W, H = 200, 120
    n = c1.shape[1]
    r = gpu.Renderer()
    away = cam_for(gpu, W, H, pos=(0, 0, 4), look=(0, 0, 8))     # looking away from the cloud
    for kw in (dict(cam=cam_for(gpu, W, H), n=0), dict(cam=away)):
        b = new_bufs(torch, n, W, H, fill=(5, 6, 9))
        contrib_into(gpu, torch, r, scene1, kw["cam"], W, H, b, n=kw.get("n"))
        h = to_host(b)
        assert (h["count"] == 5).all() and (h["weight"] == 6).all() and (h["max"] == 9).all()
        assert (h["id"] == -1).all()


def test_4d_scene(gpu, torch, tmp_path_factory):
    """A 4D scene at t = 0.3: the id plane is set exactly where render_aux's alpha is."""
    p = tmp_path_factory.mktemp("contrib4d") / "scene4d.ply"
    gpu.write_synthetic_ply4d(str(p), 4_000, 5)
    soa49 = gpu.read_ply(str(p), four_d=True)
    n = soa49.shape[1]
    W, H = 320, 200
    cam = cam_for(gpu, W, H)
    scene = gpu.Scene.from_soa(soa49)
    assert scene.is_4d
    r = gpu.Renderer()
    got = contrib(gpu, torch, scene, cam, W, H, renderer=r, time=0.3)
    assert got["count"].astype(np.int64).sum() > 1000
    assert ((got["id"] >= -1) & (got["id"] < n)).all()
    alpha = torch.full((H, W), float("nan"), dtype=torch.float32, device="cuda")
    for _ in range(3):
        r.render_aux(scene, cam, W, H, alpha_ptr=alpha.data_ptr(), time=0.3)
        if r.sync() == 0:
            break
    assert np.array_equal(got["id"] >= 0, alpha.cpu().numpy() > 0)
