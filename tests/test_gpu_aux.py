"""Auxiliary render targets (gsr_render_aux, Renderer.render_aux): accumulated alpha,
un-normalised depth and composited per-Gaussian feature channels, against the UNMODIFIED
CPU oracle, bit for bit.

The oracle only renders colours, but its colour is clamp(C0 f_dc + 0.5 (+ higher SH
bands), 0, 1) per channel: a copy of the scene with f_rest (SoA arrays 14..37) zeroed and
chosen f_dc (arrays 11..13) gives any per-Gaussian "colour" over the same geometry, hence
the same composited splats, and every aux channel accumulates exactly like a colour
(acc = fma(v alpha, T, acc) in list order).  So alpha is the oracle's image of an
all-ones colour, and a feature plane fed with the oracle's own preprocessed colours of a
recoloured scene is that scene's image."""
import numpy as np
import pytest

from conftest import assert_frames, scene_soa
from test_gpu_parity import CAMS, cam_for

pytestmark = pytest.mark.gpu

SIZES = [(640, 480), (333, 217), (37, 23), (1, 1)]
# (W, H, camera): every camera at the full size, every size with the camera the blend
# mapping tests use; lists longer than two batches, odd survivor counts, blocks cut by
# the image edge, saturated and never-saturated pixels, empty tiles
CASES = [(640, 480, ci) for ci in range(len(CAMS))] + [(W, H, 1) for W, H in SIZES[1:]]
TILINGS = [(8, 8, 40, 30), (7, 3, 92, 160)]
# ... and _wide_scenes' tilted scene from camera 0 (the third entry names the scene): random
# quaternions, so the conics carry off-diagonal terms of their own, up to 81 takes per pixel
WIDE_CASES = [(128, 80, "tilted")]
F_DC, F_REST = slice(11, 14), slice(14, 38)


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


def ones_soa(soa):
    """Every Gaussian's red is clamp(C0 * 4 + 0.5) = 1.0f exactly."""
    s = soa.copy()
    s[F_REST] = 0.0
    s[11] = 4.0
    return s


def random_soa(soa, seed=7):
    """f_dc uniform in [-3, 3]: colours C0 f_dc + 0.5 in about [-0.35, 1.35], so the clamps
    hit at both ends."""
    s = soa.copy()
    s[F_REST] = 0.0
    s[F_DC] = np.random.default_rng(seed).uniform(-3.0, 3.0, (3, soa.shape[1])).astype(np.float32)
    return s


_refs = {}


def cam_of(gsr, W, H, ci):
    """The camera of a case: CAMS[ci], or camera 0 where ci names a scene of WIDE_CASES."""
    return cam_for(gsr, W, H, **CAMS[ci if isinstance(ci, int) else 0])


@pytest.fixture(scope="module")
def scene_of(gpu, c1, scene1):
    """ci -> (arrays, scene) of a case: config 1, or the scene that ci names."""
    cache = {}

    def get(ci):
        if isinstance(ci, int):
            return c1, scene1
        if ci not in cache:
            from _wide_scenes import scene as wide_scene
            cache[ci] = (wide_scene(ci), gpu.Scene.from_soa(wide_scene(ci)))
        return cache[ci]
    return get


def oracle(orc, gsr, kind, soa, W, H, ci, tiling=None):
    """The oracle's images, computed once per module: 'rgb' the scene's, 'ones' channel 0 of
    the all-ones recolouring (= alpha), 'rand' the random recolouring's, with the
    preprocessed colours (3, n) that make it up."""
    key = (kind, W, H, ci, tiling)
    if key not in _refs:
        cam = cam_of(gsr, W, H, ci)
        if kind == "rgb":
            _refs[key] = orc.render(soa, cam, W, H, 3.0, tiling=tiling)
        elif kind == "ones":
            _refs[key] = orc.render(ones_soa(soa), cam, W, H, 3.0, tiling=tiling)[0].copy()
        else:
            s2 = random_soa(soa)
            feat = np.ascontiguousarray(orc.preprocess(s2, cam, W, H, 3.0)["color"].T)
            _refs[key] = (orc.render(s2, cam, W, H, 3.0, tiling=tiling), feat)
    return _refs[key]


def tiling_of(gsr, W, H, tiling):
    if tiling is None:
        return None
    t = gsr.TilingInformation(1, 1, H, W)
    t.num_tile_x, t.num_tile_y, t.width_stride, t.height_stride = tiling
    return t


def aux(gsr, torch, scene, cam, W, H, out=True, alpha=True, depth=True, feats=None, tiling=None, renderer=None,
        n=None, time=None):
    """One aux frame; returns {"out": (3, H, W), "alpha": (H, W), "depth": (H, W), "feat":
    (nfeat, H, W)} of the requested planes.  Every buffer starts as NaN: a pixel the frame
    leaves unwritten fails any comparison."""
    r = renderer or gsr.Renderer()
    nan = float("nan")
    nfeat = 0 if feats is None else feats.shape[0]
    b = {}
    if out:
        b["out"] = torch.full((3, H, W), nan, dtype=torch.float32, device="cuda")
    if alpha:
        b["alpha"] = torch.full((H, W), nan, dtype=torch.float32, device="cuda")
    if depth:
        b["depth"] = torch.full((H, W), nan, dtype=torch.float32, device="cuda")
    d_feat = None
    if nfeat:
        d_feat = torch.from_numpy(np.ascontiguousarray(feats, dtype=np.float32)).cuda()
        b["feat"] = torch.full((nfeat, H, W), nan, dtype=torch.float32, device="cuda")
    ptr = lambda k: b[k].data_ptr() if k in b else None   # noqa: E731
    for _ in range(3):
        r.render_aux(scene, cam, W, H, out_ptr=ptr("out"), alpha_ptr=ptr("alpha"), depth_ptr=ptr("depth"),
                     features_ptr=d_feat.data_ptr() if nfeat else None, nfeat=nfeat, feat_out_ptr=ptr("feat"),
                     tiling=tiling_of(gsr, W, H, tiling), n=n, time=time)
        if r.sync() == 0:
            break
    else:
        raise AssertionError("aux frame still incomplete after three renders")
    return {k: v.cpu().numpy() for k, v in b.items()}


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def plain(gsr, torch, scene, cam, W, H, renderer):
    out = torch.empty(3 * W * H, dtype=torch.float32, device="cuda")
    for _ in range(3):
        renderer.render(scene, cam, W, H, out.data_ptr())
        if renderer.sync() == 0:
            break
    return out.view(3, H, W).cpu().numpy()


# ---------------------------------------------------------------- 1. colour, 2. alpha

@pytest.mark.parametrize("W,H,ci", CASES + WIDE_CASES)
def test_colour_and_alpha_match_oracle(gpu, orc, torch, scene_of, W, H, ci):
    """d_out is the oracle's image bit for bit with knob 22 at its default (aux frames
    always run the exact blend); alpha is the oracle's image of an all-ones colour; a plain
    render() on the same context afterwards is unaffected."""
    c1, scene1 = scene_of(ci)
    cam = cam_of(gpu, W, H, ci)
    r = gpu.Renderer()
    got = aux(gpu, torch, scene1, cam, W, H, renderer=r)
    want = oracle(orc, gpu, "rgb", c1, W, H, ci)
    assert same_bits(got["out"], want)
    a = oracle(orc, gpu, "ones", c1, W, H, ci)
    if (W, H, ci) in ((640, 480, 3), (333, 217, 1)):
        # these cases exercise saturation (T < 1e-3 <=> alpha > 0.999) and partial coverage
        # (the other cameras' full-size images peak just below 0.999; 37 x 23 is mostly
        # saturated)
        assert (a != 0).sum() > 1000 and (a >= 0.999).any() and ((a > 0) & (a < 0.5)).any()
    assert same_bits(got["alpha"], a)
    assert_frames(plain(gpu, torch, scene1, cam, W, H, r), want)


# ---------------------------------------------------------------- 3. features

@pytest.mark.parametrize("W,H,ci,tiling", [c + (None,) for c in CASES] + [(640, 480, 1, t) for t in TILINGS])
def test_features_match_recoloured_oracle(gpu, orc, torch, c1, scene1, W, H, ci, tiling):
    """The GPU scene is the ORIGINAL one; the features are the oracle's preprocessed colours
    of the recoloured scene: the feature planes are that scene's image bit for bit."""
    cam = cam_for(gpu, W, H, **CAMS[ci])
    want, feat = oracle(orc, gpu, "rand", c1, W, H, ci, tiling)
    assert feat.shape == (3, c1.shape[1]) and (feat == 0).any() and (feat == 1).any()
    got = aux(gpu, torch, scene1, cam, W, H, out=False, depth=False, feats=feat, tiling=tiling)
    assert same_bits(got["feat"], want)
    assert same_bits(got["alpha"], oracle(orc, gpu, "ones", c1, W, H, ci, tiling))


# ---------------------------------------------------------------- 4. depth

def depth_values(orc, gsr, soa, W, H, ci):
    spl = orc.preprocess(soa, cam_of(gsr, W, H, ci), W, H, 3.0)
    vis = spl["status"] == 2
    return np.where(vis, -spl["view"][:, 2], np.float32(0)).astype(np.float32), vis


@pytest.mark.parametrize("W,H,ci", CASES + WIDE_CASES)
def test_depth_is_the_feature_of_view_z(gpu, orc, torch, scene_of, W, H, ci):
    """The depth plane equals the feature plane of zf = -view z (the oracle's, 0 for
    culled Gaussians) bit for bit: the stored value is the oracle's float, composited like
    any other channel.  Where alpha >= 0.5 the expected depth lies within the visible
    splats' range, widened by 2^-20 relative (far above the fma chain's rounding, a few
    hundred takes x 2^-24: the bound only catches gross errors)."""
    c1, scene1 = scene_of(ci)
    cam = cam_of(gpu, W, H, ci)
    zf, vis = depth_values(orc, gpu, c1, W, H, ci)
    d = aux(gpu, torch, scene1, cam, W, H, out=False, alpha=False)["depth"]
    f = aux(gpu, torch, scene1, cam, W, H, out=False, alpha=False, depth=False, feats=zf[None])["feat"][0]
    assert same_bits(d, f)
    a = oracle(orc, gpu, "ones", c1, W, H, ci)
    m = a >= 0.5
    if vis.any() and m.any():
        e = d[m].astype(np.float64) / a[m].astype(np.float64)
        lo, hi = float(zf[vis].min()), float(zf[vis].max())
        assert lo > 0
        assert (e >= lo * (1 - 2.0 ** -20)).all() and (e <= hi * (1 + 2.0 ** -20)).all()
    if (W, H) == (640, 480):
        assert m.sum() > 1000


def test_depth_of_one_opaque_gaussian(gpu, orc, torch):
    """n = 1: at the Gaussian's centre pixel depth / alpha is its -view z within 2^-22."""
    soa = np.zeros((38, 1), np.float32)
    soa[0:3, 0] = (0.1, -0.2, 0.3)
    soa[3, 0] = 0.95                      # opacity
    soa[4:7, 0] = 0.2                     # scale
    soa[7, 0] = 1.0                       # identity rotation
    W, H = 64, 48
    cam = cam_for(gpu, W, H)
    spl = orc.preprocess(soa, cam, W, H, 3.0)
    assert spl["status"][0] == 2
    zf = float(-spl["view"][0, 2])
    got = aux(gpu, torch, gpu.Scene.from_soa(soa), cam, W, H, out=False)
    x, y = int(spl["px_x"][0]), int(spl["px_y"][0])
    a, d = float(got["alpha"][y, x]), float(got["depth"][y, x])
    assert a > 0.9
    assert abs(d / a - zf) <= 2.0 ** -22 * zf


# ---------------------------------------------------------------- 5. NF and NULL combinations

def test_feature_counts_and_null_outputs(gpu, torch, c1, scene1):
    W, H = 333, 217
    cam = cam_for(gpu, W, H, **CAMS[1])
    n = c1.shape[1]
    feats = np.random.default_rng(11).uniform(-3.0, 3.0, (8, n)).astype(np.float32)
    r = gpu.Renderer()
    full = aux(gpu, torch, scene1, cam, W, H, feats=feats, renderer=r)
    assert (full["alpha"] > 0).sum() > 1000
    for nf in (0, 1, 3, 8):
        f = feats[:nf] if nf else None
        for drop in ("out", "alpha", "depth"):
            keep = {k: k != drop for k in ("out", "alpha", "depth")}
            got = aux(gpu, torch, scene1, cam, W, H, feats=f, renderer=r, **keep)
            assert set(got) == {k for k, v in keep.items() if v} | ({"feat"} if nf else set())
            for k in ("out", "alpha", "depth"):
                if keep[k]:
                    assert same_bits(got[k], full[k]), (nf, drop, k)
            if nf:
                assert same_bits(got["feat"], full["feat"][:nf]), (nf, drop)
    # features only, and each array of the 8-feature call rendered alone
    for j in range(8):
        got = aux(gpu, torch, scene1, cam, W, H, out=False, alpha=False, depth=False, feats=feats[j:j + 1],
                  renderer=r)
        assert set(got) == {"feat"} and same_bits(got["feat"][0], full["feat"][j]), j


# ---------------------------------------------------------------- 6. frame policy

KNOB_SPLIT, KNOB_PM, KNOB_STATE = 23, 24, 26


def test_depth_split_controller_untouched(gpu, orc, torch, c1, scene1):
    """With the depth split forced on, an aux frame still runs one exact phase (outputs
    unchanged) and leaves the split point and the last frame's split state as they were;
    plain frames before and after it match the oracle."""
    W, H, ci = 640, 480, 0
    cam = cam_for(gpu, W, H, **CAMS[ci])
    want = oracle(orc, gpu, "rgb", c1, W, H, ci)
    r = gpu.Renderer()
    r.set_tuning(KNOB_SPLIT, 1)
    r.set_tuning(KNOB_PM, 150)
    for _ in range(2):   # the second split frame runs in key mode
        assert_frames(plain(gpu, torch, scene1, cam, W, H, r), want)
    assert r.sync() == 0
    pm, state = r.get_tuning(KNOB_PM), r.get_tuning(KNOB_STATE)
    assert state != 0
    got = aux(gpu, torch, scene1, cam, W, H, renderer=r)
    assert same_bits(got["out"], want)
    assert same_bits(got["alpha"], oracle(orc, gpu, "ones", c1, W, H, ci))
    assert (r.get_tuning(KNOB_PM), r.get_tuning(KNOB_STATE)) == (pm, state)
    assert_frames(plain(gpu, torch, scene1, cam, W, H, r), want)
    assert r.get_tuning(KNOB_STATE) != 0


def test_aux_first_frame_with_split_on(gpu, orc, torch, c1, scene1):
    """Knobs 23 = 1 and 24 = 150 on a fresh context: the aux frame's outputs are the
    one-phase ones, the knobs read back unchanged, a plain render() afterwards matches."""
    W, H, ci = 640, 480, 1
    cam = cam_for(gpu, W, H, **CAMS[ci])
    r = gpu.Renderer()
    r.set_tuning(KNOB_SPLIT, 1)
    r.set_tuning(KNOB_PM, 150)
    before = (r.get_tuning(KNOB_PM), r.get_tuning(KNOB_STATE))
    got = aux(gpu, torch, scene1, cam, W, H, renderer=r)
    assert same_bits(got["out"], oracle(orc, gpu, "rgb", c1, W, H, ci))
    assert same_bits(got["alpha"], oracle(orc, gpu, "ones", c1, W, H, ci))
    assert (r.get_tuning(KNOB_PM), r.get_tuning(KNOB_STATE)) == before == (150, 0)
    assert_frames(plain(gpu, torch, scene1, cam, W, H, r), oracle(orc, gpu, "rgb", c1, W, H, ci))


@pytest.mark.parametrize("knobs", [{13: 0}, {13: 64}, {7: 0}, {28: 0}])
def test_knobs_do_not_change_aux_outputs(gpu, orc, torch, c1, scene1, knobs):
    """Block mappings (13), the pair-sort path (7 = 0) and the LSD depth sort (28 = 0)."""
    for W, H in ((640, 480), (37, 23)):
        ci = 1
        cam = cam_for(gpu, W, H, **CAMS[ci])
        want, feat = oracle(orc, gpu, "rand", c1, W, H, ci)
        r = gpu.Renderer()
        for kn, v in knobs.items():
            r.set_tuning(kn, v)
        for _ in range(2):   # the second frame of a context takes the bucket sort (28)
            got = aux(gpu, torch, scene1, cam, W, H, feats=feat, renderer=r)
            assert same_bits(got["out"], oracle(orc, gpu, "rgb", c1, W, H, ci))
            assert same_bits(got["alpha"], oracle(orc, gpu, "ones", c1, W, H, ci))
            assert same_bits(got["feat"], want)


# ---------------------------------------------------------------- 7. edge cases

def test_empty_and_all_culled(gpu, torch, c1, scene1):
    W, H = 200, 120
    feats = np.ones((2, c1.shape[1]), np.float32)
    cam = cam_for(gpu, W, H)
    got = aux(gpu, torch, scene1, cam, W, H, feats=feats, n=0)
    away = cam_for(gpu, W, H, pos=(0, 0, 4), look=(0, 0, 8))     # looking away from the cloud
    got2 = aux(gpu, torch, scene1, away, W, H, feats=feats)
    for g in (got, got2):
        assert set(g) == {"out", "alpha", "depth", "feat"}
        for k, v in g.items():
            assert not v.view(np.uint32).any(), k


def test_4d_scene_alpha(gpu, orc, torch, tmp_path_factory):
    """A 4D scene at t = 0.3: alpha against the oracle on the scene at that time (no
    temporal cull there: the GPU's cull only drops Gaussians that cannot composite),
    recoloured to ones; the tolerance tests/test_gpu_4d.py uses for colours."""
    p = tmp_path_factory.mktemp("aux4d") / "scene4d.ply"
    gpu.write_synthetic_ply4d(str(p), 4_000, 5)
    soa49 = gpu.read_ply(str(p), four_d=True)
    W, H = 320, 200
    cam = cam_for(gpu, W, H)
    scene = gpu.Scene.from_soa(soa49)
    assert scene.is_4d
    got = aux(gpu, torch, scene, cam, W, H, out=False, time=0.3)
    want = orc.render(ones_soa(orc.temporal(soa49, 0.3)), cam, W, H, 3.0)[0]
    assert (want != 0).sum() > 1000
    assert_frames(got["alpha"], want)
    assert np.isfinite(got["depth"]).all() and ((got["depth"] > 0) == (got["alpha"] > 0)).all()


def test_pair_overflow_grows_and_rerenders(gpu, orc, torch):
    """Huge splats (tests/test_gpu_parity.py's): the first aux frame overflows the pair
    buffer, sync() reports it, and the re-render is complete and correct."""
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
    out = torch.empty(3 * W * H, device="cuda")
    alpha = torch.empty(W * H, device="cuda")
    r.render_aux(scene, cam, W, H, out_ptr=out.data_ptr(), alpha_ptr=alpha.data_ptr())
    assert r.sync() == -5                      # overflow reported and buffer grown
    r.render_aux(scene, cam, W, H, out_ptr=out.data_ptr(), alpha_ptr=alpha.data_ptr())
    assert r.sync() == 0
    assert r.pair_count() > 1_000_000
    assert same_bits(out.view(3, H, W).cpu().numpy(), orc.render(soa, cam, W, H, 3.0))
    assert same_bits(alpha.view(H, W).cpu().numpy(), orc.render(ones_soa(soa), cam, W, H, 3.0)[0])


# ---------------------------------------------------------------- 8. determinism

def test_two_aux_frames_give_identical_bytes(gpu, torch, c1, scene1):
    W, H = 640, 480
    cam = cam_for(gpu, W, H, **CAMS[1])
    feats = np.random.default_rng(3).uniform(-3.0, 3.0, (5, c1.shape[1])).astype(np.float32)
    r = gpu.Renderer()
    a = aux(gpu, torch, scene1, cam, W, H, feats=feats, renderer=r)
    b = aux(gpu, torch, scene1, cam, W, H, feats=feats, renderer=r)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


# ---------------------------------------------------------------- 9. a workspace that grows in a live context

def test_workspace_regrows(gpu, torch, tmp_path_factory):
    """One context, no gsr_reserve: 500 Gaussians on 64 x 48, then 3,000 on 160 x 96 (past the
    1,024-element floor of the per-Gaussian buffers, and a larger tile grid), then the small size
    again.  At each step a plain frame, an aux frame with depth and 6 features (aux_z and
    aux_pack), the fused backward call without a caller's scratch (rec_grads), an AoS-layout frame
    (soa_tmp) and a frame with the depth split forced on (tbuf, bflag).  Each result equals, bit
    for bit, the same call on a fresh context at that size.

    The backward call's upstream gradient is non-zero at two pixels only: the blend's backward
    pass sums a Gaussian's record gradients over pixels with float atomics in no fixed order, and
    a sum of at most two terms is the same in either order, so the comparison can be exact."""
    from gaussianrenderer_amd import _native
    from test_gpu_parity import aos_records
    sizes = {"small": (500, 64, 48), "large": (3000, 160, 96)}
    data = {}
    for name, (n, W, H) in sizes.items():
        soa = scene_soa(gpu, tmp_path_factory, n, 3)[1]
        data[name] = dict(n=n, W=W, H=H, cam=cam_for(gpu, W, H), scene=gpu.Scene.from_soa(soa),
                          aos=torch.from_numpy(aos_records(soa)).cuda(),
                          feats=np.random.default_rng(n).uniform(-3.0, 3.0, (6, n)).astype(np.float32))

    def synced(r, call):
        for _ in range(3):
            call()
            if r.sync() == 0:
                return
        raise AssertionError("frame still incomplete after three renders")

    def image(r, d, **kw):
        out = torch.full((3, d["H"], d["W"]), float("nan"), dtype=torch.float32, device="cuda")
        scene = kw.pop("scene", d["scene"])
        synced(r, lambda: r.render(scene, d["cam"], d["W"], d["H"], out.data_ptr(), **kw))
        return {"out": out.cpu().numpy()}

    def backward(r, d):
        n = d["n"]
        planes = {k: torch.zeros(c * n, dtype=torch.float32, device="cuda")
                  for k, c in (("position", 3), ("opacity", 1), ("scale", 3), ("rot", 4), ("sh", 27))}

        def call():
            for p in planes.values():
                p.zero_()
            r.render_backward_scene(d["scene"], d["cam"], d["W"], d["H"], grad_image_ptr=d["grad"],
                                    **{k + "_ptr": p for k, p in planes.items()})
        synced(r, call)
        got = {k: p.cpu().numpy() for k, p in planes.items()}
        assert got["position"].any() and got["sh"].any()
        return got

    def split(r, d):
        r.set_tuning(KNOB_SPLIT, 1)
        got = image(r, d)
        r.set_tuning(KNOB_SPLIT, 2)
        return got

    for d in data.values():   # the upstream gradient: the image's two brightest pixels, so splats cover them
        img = image(gpu.Renderer(), d)["out"].sum(0)
        g = np.zeros((3, d["H"], d["W"]), np.float32)
        for px, v in zip(np.argsort(img, axis=None)[-2:], ((1.0, -0.5, 0.25), (-0.75, 1.0, 0.5))):
            g[:, px // d["W"], px % d["W"]] = v
        d["grad"] = torch.from_numpy(g).cuda()

    calls = {
        "render": image,
        "aux": lambda r, d: aux(gpu, torch, d["scene"], d["cam"], d["W"], d["H"], feats=d["feats"], renderer=r),
        "backward": backward,
        "aos": lambda r, d: image(r, d, scene=d["aos"].data_ptr(), layout=_native.LAYOUT_AOS, n=d["n"]),
        "split": split,
    }
    fresh = {(name, k): call(gpu.Renderer(), d) for name, d in data.items() for k, call in calls.items()}
    assert (fresh["large", "render"]["out"] != 0).sum() > 1000
    live = gpu.Renderer()
    for name in ("small", "large", "small"):
        for k, call in calls.items():
            got, want = call(live, data[name]), fresh[name, k]
            assert set(got) == set(want)
            for plane in got:
                assert same_bits(got[plane], want[plane]), (name, k, plane)
