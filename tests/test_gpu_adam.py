"""gsr_scene_adam_step on the device (Scene.adam_step): x, m and v against the float32 twin
(tests/_adam_ref.py) bit for bit over every block kind, the wave-edge sizes and both element
mappings; frozen groups, guard words and the block's padding; the skipped elements and d_bad;
and what makes the call worth having: a stepped block renders through an existing context
exactly as a fresh upload of it does, and a closed render -> backward -> step loop descends."""
import numpy as np
import pytest

import _adam_ref as ref
from test_adam_ref import LRS, random_scene
from test_gpu_parity import CAMS, cam_for
from test_gpu_scene_ops import dense_soa, dev, exact_renderer, frame, same_bits

pytestmark = pytest.mark.gpu

SENT = 0x5A5A5A5A
GUARD = 64                       # sentinel words after every caller buffer
PAD_BITS = 0x7FC0BEEF            # what the crafted blocks hold in [n, stride): a NaN with a payload
MAGIC = [0x7FC0A5E1, 0x7FC05352, 0x7FC03347, 0x7FC00001]


@pytest.fixture(scope="module")
def torch(gpu):
    import torch as t
    assert t.cuda.is_available()
    return t


@pytest.fixture(scope="module")
def exp32(orc):
    return ref.orc_exp32(orc)


# ---------------------------------------------------------------- helpers

def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def upload_block(gsr, torch, soa):
    """A device scene block of soa whose padding [n, stride) holds PAD_BITS in every array: a
    crafted block image copied over a fresh upload by gsr_scene_copy."""
    narrays, n = soa.shape
    stride = (n + 63) // 64 * 64
    img = np.full((narrays, stride), PAD_BITS, np.uint32)
    img[:, :n] = bits(soa)
    hdr = np.zeros(64, np.uint32)
    hdr[:4] = MAGIC
    hdr[4:10].view(np.uint64)[:] = [n, stride, narrays]
    d_raw = dev(torch, np.concatenate([hdr, img.ravel()]))
    scene = gsr.Scene.from_soa(soa)
    assert gsr.lib().gsr_scene_bytes(narrays, n) == 4 * d_raw.numel()
    assert gsr.lib().gsr_scene_copy(scene.ptr, d_raw.data_ptr(), narrays, n, None) == 0
    torch.cuda.synchronize()
    return scene


def read_block(gsr, torch, scene):
    """The block's arrays with their padding, (narrays, stride) words."""
    nbytes = gsr.lib().gsr_scene_bytes(scene.narrays, scene.n)
    buf = torch.zeros(nbytes // 4, dtype=torch.int32, device="cuda")
    assert gsr.lib().gsr_scene_copy(buf.data_ptr(), scene.ptr, scene.narrays, scene.n, None) == 0
    torch.cuda.synchronize()
    return buf[64:].cpu().numpy().view(np.uint32).reshape(scene.narrays, -1)


def assert_block(gsr, torch, scene, want_soa, what=""):
    got = read_block(gsr, torch, scene)
    n = scene.n
    assert (got[:, n:] == PAD_BITS).all(), f"{what}: the block's padding was written"
    diff = got[:, :n] != bits(want_soa)
    assert not diff.any(), f"{what}: x differs from the twin at (array, i) {np.argwhere(diff)[:8].tolist()}"


class DevPlanes:
    """A dict of host plane groups on the device, each buffer `off` sentinel words, the planes,
    then GUARD sentinel words; off = 1 puts every plane on an address that is 4 mod 16."""

    def __init__(self, torch, host, off=0):
        self.off, self.buf, self.ptr, self.shape = off, {}, {}, {}
        for k, a in host.items():
            if a is None:
                continue
            t = torch.full((off + a.size + GUARD,), SENT, dtype=torch.int32, device="cuda")
            t[off:off + a.size].copy_(torch.from_numpy(bits(a).view(np.int32).reshape(-1)))
            self.buf[k], self.ptr[k], self.shape[k] = t, t.data_ptr() + 4 * off, a.shape
            assert self.ptr[k] % 16 == 4 * off

    def host(self):
        """The planes back on the host as float32; the sentinels must be intact."""
        out = {}
        for k, t in self.buf.items():
            w = t.cpu().numpy().view(np.uint32)
            size = int(np.prod(self.shape[k]))
            assert (w[:self.off] == SENT).all() and (w[self.off + size:] == SENT).all(), f"guard words of {k} written"
            out[k] = w[self.off:self.off + size].view(np.float32).reshape(self.shape[k]).copy()
        return out


def log_uniform(rng, shape, lo=-8.0, hi=3.0):
    return (10.0 ** rng.uniform(lo, hi, shape)).astype(np.float32)


def random_state(narrays, n, rng):
    """A scene, gradients with magnitudes from 1e-8 to 1e3 and the non-zero moments an earlier
    step left (v >= 0), all float32."""
    soa = random_scene(narrays, n, rng).astype(np.float32)
    soa[3, :min(n, 3)] = np.array([1e-6, 0.999999, 0.5], np.float32)[:min(n, 3)]   # the clamp's ends
    keys = [k for k in ref.GROUP_KEYS if k != "temporal" or narrays == 49]
    P = ref.planes_of(narrays)
    g = {k: log_uniform(rng, (P[k], n)) * rng.choice(np.float32([-1, 1]), (P[k], n)) for k in keys}
    m = {k: log_uniform(rng, (P[k], n)) * rng.choice(np.float32([-1, 1]), (P[k], n)) for k in keys}
    v = {k: log_uniform(rng, (P[k], n)) ** 2 * rng.uniform(0.1, 1, (P[k], n)).astype(np.float32) for k in keys}
    for d in (g, m, v):
        assert all(a.dtype == np.float32 and (a != 0).all() for a in d.values())
    return soa, g, m, v


def assert_planes(got, want, what):
    assert set(got) == set(want)
    for k in want:
        diff = bits(got[k]) != bits(want[k])
        assert not diff.any(), f"{what}[{k}] differs from the twin at (plane, i) {np.argwhere(diff)[:8].tolist()}"


def run_step(gsr, torch, soa, g, m, v, lrs, step, off=0, bad=False, **flags):
    """One device step on fresh buffers: (scene, g, m, v back on the host, d_bad or None)."""
    scene = upload_block(gsr, torch, soa)
    dg, dm, dv = (DevPlanes(torch, d, off) for d in (g, m, v))
    d_bad = torch.zeros(1, dtype=torch.int32, device="cuda") if bad else None
    scene.adam_step(dg.ptr, dm.ptr, dv.ptr, step=step, bad_ptr=d_bad, **lrs, **flags)
    torch.cuda.synchronize()
    return scene, dg.host(), dm.host(), dv.host(), (int(d_bad.item()) if bad else None)


def check_against_twin(gsr, torch, exp32, soa, g, m, v, lrs, step, off=0, bad=False, skip_zero=False,
                       zero_grads=False):
    want = ref.adam_step(soa, g, m, v, lrs, step, exp32, skip_zero=skip_zero, zero_grads=zero_grads)
    scene, g2, m2, v2, nbad = run_step(gsr, torch, soa, g, m, v, lrs, step, off, bad, skip_zero=skip_zero,
                                       zero_grads=zero_grads)
    what = f"n={soa.shape[1]} narrays={soa.shape[0]} step={step} off={off}"
    assert_block(gsr, torch, scene, want[0], what)
    assert_planes(m2, want[2], "m " + what)
    assert_planes(v2, want[3], "v " + what)
    if zero_grads:
        for k in g2:                                   # +-0 where cleared, the bits it had elsewhere
            zero = want[1][k] == 0
            assert (g2[k][zero] == 0).all() and np.array_equal(bits(g2[k])[~zero], bits(want[1][k])[~zero]), \
                f"g[{k}] {what}"
    else:
        assert_planes(g2, g, "g " + what)                                            # read-only
    if bad:
        assert nbad == want[4], what
    return want, scene


# ---------------------------------------------------------------- 1. bit-exact against the twin

CASES = [(n, na) for n in (1, 63, 64, 65, 4097, 10_000) for na in (38, 59)] + [(65, 49), (4097, 49)]


@pytest.mark.parametrize("n,narrays", CASES)
def test_bit_exact(gpu, torch, exp32, n, narrays):
    """Every group active, at step 1 and step 1000, from 16-byte aligned buffers (n = 64 and
    10,000: every plane takes the 16-byte accesses; other n: the planes whose c*n is no multiple
    of 4 take the 4-byte mapping) and from buffers offset by 4 bytes (the other way round)."""
    rng = np.random.default_rng(1000 * narrays + n)
    soa, g, m, v = random_state(narrays, n, rng)
    for step, off in ((1, 0), (1, 1), (1000, 0), (1000, 1)):
        want, _ = check_against_twin(gpu, torch, exp32, soa, g, m, v, LRS, step, off)
        moved = bits(want[0]) != bits(soa)
        assert moved.mean() > 0.5, "the step moved too little to compare"


def test_determinism(gpu, torch):
    soa, g, m, v = random_state(49, 4097, np.random.default_rng(3))
    runs = []
    for _ in range(2):
        scene, g2, m2, v2, _ = run_step(gpu, torch, soa, g, m, v, LRS, 7, off=1)
        runs.append((read_block(gpu, torch, scene), m2, v2))
    assert np.array_equal(runs[0][0], runs[1][0])
    assert_planes(runs[0][1], runs[1][1], "m")
    assert_planes(runs[0][2], runs[1][2], "v")


# ---------------------------------------------------------------- 2. frozen groups

@pytest.mark.parametrize("narrays", [38, 49])
def test_frozen_groups(gpu, torch, exp32, narrays):
    """Only position and sh_dc are stepped, every other pointer NULL: the other arrays of the
    block, and the sh_rest planes of g, m and v, keep their bits."""
    n = 1029
    soa, g, m, v = random_state(narrays, n, np.random.default_rng(narrays))
    only = lambda d: {k: d[k] for k in ("position", "sh")}
    lrs = {"lr_position": 1e-3, "lr_sh_dc": 2e-3}
    want, scene = check_against_twin(gpu, torch, exp32, soa, only(g), only(m), only(v), lrs, 3, zero_grads=True)
    got = read_block(gpu, torch, scene)[:, :n]
    stepped = [0, 1, 2, 11, 12, 13]
    frozen = [a for a in range(narrays) if a not in stepped]
    assert np.array_equal(got[frozen], bits(soa)[frozen])
    assert (got[stepped] != bits(soa)[stepped]).mean() > 0.5
    # the twin left the frozen planes of "sh" alone too, and check_against_twin compared them:
    assert same_bits(want[1]["sh"][3:], g["sh"][3:]) and not want[1]["sh"][:3].any()


# ---------------------------------------------------------------- 3. skipping, d_bad, ZERO_GRADS

def plant_bad(g, n, rng):
    """NaN, +inf and -inf at known elements, the first and last element of a plane among them;
    returns their number."""
    vals = np.float32([np.nan, np.inf, -np.inf])
    count = 0
    for k, a in g.items():
        for p in range(a.shape[0]):
            idx = np.unique(np.concatenate([[0, n - 1], rng.integers(0, n, 5)])) if p % 2 == 0 else rng.integers(0, n, 3)
            idx = np.unique(idx)
            a[p, idx] = vals[rng.integers(0, 3, idx.size)]
            count += idx.size
    return count


@pytest.mark.parametrize("n,narrays,off", [(4097, 38, 0), (4097, 49, 1), (1000, 59, 0), (64, 38, 1)])
def test_non_finite_gradients_are_skipped_and_counted(gpu, torch, exp32, n, narrays, off):
    rng = np.random.default_rng(n + narrays)
    soa, g, m, v = random_state(narrays, n, rng)
    planted = plant_bad(g, n, rng)
    for zero_grads in (False, True):
        want, scene = check_against_twin(gpu, torch, exp32, soa, g, m, v, LRS, 2, off, bad=True,
                                         zero_grads=zero_grads)
        assert want[4] == planted
        # untouched where the gradient was not finite (the twin agrees, and is compared above)
        got = read_block(gpu, torch, scene)[:, :n]
        for key, first, planes, array, _, _ in ref.groups(narrays):
            skip = ~np.isfinite(g[key][first:first + planes])
            assert np.array_equal(got[array:array + planes][skip], bits(soa)[array:array + planes][skip])
    # without a counter the same elements arrive
    check_against_twin(gpu, torch, exp32, soa, g, m, v, LRS, 2, off)


@pytest.mark.parametrize("n,narrays,off", [(4097, 38, 0), (4097, 49, 1), (10_000, 59, 0), (10_000, 38, 1)])
def test_skip_zero(gpu, torch, exp32, n, narrays, off):
    """A random 70 % of whole Gaussians with zero gradients, Gaussians [1024, 2048) all zero
    (whole waves leave early under either mapping), a few isolated +-0 elements and a NaN."""
    rng = np.random.default_rng(7 * n + narrays)
    soa, g, m, v = random_state(narrays, n, rng)
    dead = rng.random(n) < 0.7
    dead[1024:2048] = True
    for a in g.values():
        a[:, dead] = 0
        for p in range(a.shape[0]):
            a[p, rng.integers(0, n, 4)] = np.float32([0.0, -0.0, 0.0, -0.0])
    g["position"][1, [0, n - 1]] = [-0.0, 0.0]
    g["rot"][3, n // 2] = np.nan
    for zero_grads in (False, True):
        want, scene = check_against_twin(gpu, torch, exp32, soa, g, m, v, LRS, 5, off, bad=True, skip_zero=True,
                                         zero_grads=zero_grads)
        assert want[4] == 1
        got = read_block(gpu, torch, scene)[:, :n]
        for key, first, planes, array, _, _ in ref.groups(narrays):
            zero = g[key][first:first + planes] == 0
            assert zero.mean() > 0.65
            assert np.array_equal(got[array:array + planes][zero], bits(soa)[array:array + planes][zero])
            assert (got[array:array + planes][~zero] != bits(soa)[array:array + planes][~zero]).mean() > 0.5
    # the dense step of the same gradients moves the zero elements' moments (they decay)
    dense = ref.adam_step(soa, g, m, v, LRS, 5, exp32)
    assert (bits(dense[2]["position"]) != bits(want[2]["position"])).mean() > 0.65


# ---------------------------------------------------------------- 4. coherence with the renderer

W = H = 64
ALL_LRS = {"lr_position": 1e-3, "lr_opacity": 0.05, "lr_scale": 5e-3, "lr_rot": 1e-3, "lr_sh_dc": 2.5e-3,
           "lr_sh_rest": 1e-3}


def zeros_like_groups(torch, n, keys=("position", "opacity", "scale", "rot", "sh")):
    P = ref.planes_of(38)
    return {k: torch.zeros(P[k] * n, dtype=torch.float32, device="cuda") for k in keys}


def backward_frame(torch, r, scene, cam, grad_image, grads):
    """One complete render_backward_scene frame accumulated into grads (an incomplete frame
    adds nothing, so it is simply rendered again)."""
    for _ in range(3):
        r.render_backward_scene(scene, cam, W, H, grad_image_ptr=grad_image,
                                **{k + "_ptr": t for k, t in grads.items()})
        if r.sync() == 0:
            return
    raise AssertionError("backward frame still incomplete after three renders")


def test_stepped_block_renders_through_an_existing_context(gpu, orc, torch):
    soa = dense_soa()
    n = soa.shape[1]
    scene = gpu.Scene.from_soa(soa)
    cam = cam_for(gpu, W, H, **CAMS[0])
    r = exact_renderer(gpu)
    grad_image = dev(torch, np.random.default_rng(4).normal(0, 1, 3 * W * H).astype(np.float32))
    g, m, v = (zeros_like_groups(torch, n) for _ in range(3))
    before = frame(gpu, torch, r, scene, cam, W, H)
    step = 0

    def train(steps):
        nonlocal step
        for _ in range(steps):
            step += 1
            backward_frame(torch, r, scene, cam, grad_image, g)
            assert all(bool((t != 0).any()) for t in g.values())
            scene.adam_step(g, m, v, step=step, zero_grads=True, **ALL_LRS)
            assert all(not bool(t.any()) for t in g.values())

    def check(what):
        got = frame(gpu, torch, r, scene, cam, W, H)          # the same pointer, the same context
        now = scene.download()
        fresh = frame(gpu, torch, exact_renderer(gpu), gpu.Scene.from_soa(now), cam, W, H)
        assert same_bits(got, fresh), what
        assert same_bits(got, orc.render(now, cam, W, H, 3.0)), what
        return got, now

    train(1)
    img1, soa1 = check("after one step")
    assert (img1 != before).mean() > 0.5 and (soa1 != soa).mean() > 0.5
    train(3)
    img4, soa4 = check("after four steps")
    assert (img4 != img1).mean() > 0.5

    # the camera path with four frames in flight (the shared preprocess): frames before and
    # after a step, each against the oracle's image of the block as it then stands
    r.set_frames_in_flight(4)
    cams = [cam_for(gpu, W, H, **c) for c in CAMS]
    outs = [torch.full((3 * W * H,), float("nan"), dtype=torch.float32, device="cuda") for _ in cams]

    def path(what):
        for _ in range(3):
            r.render_path(scene, cams, W, H, [o.data_ptr() for o in outs])
            if r.sync() == 0:
                break
        else:
            raise AssertionError("path frames still incomplete after three renders")
        now = scene.download()
        for c, o in zip(cams, outs):
            assert same_bits(o.view(3, H, W).cpu().numpy(), orc.render(now, c, W, H, 3.0)), what

    path("path before the step")
    train(1)
    path("path after the step")
    assert (scene.download() != soa4).mean() > 0.5


def test_descent(gpu, torch):
    """Re-fitting sh_dc and the opacities to the scene's own render from a perturbed start:
    the squared error must fall (a sign error in a chain factor or in the step makes it rise).
    Nothing tighter is asserted: any figure would be measured against the code under test."""
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
    assert frame(gpu, torch, r, scene, cam, W, H) is not None   # grows the context's buffers
    sse = []
    for it in range(1, 41):
        r.render(scene, cam, W, H, image.data_ptr())
        grad = image - target
        sse.append(float((grad * grad).sum().item()))
        r.render_backward_scene(scene, cam, W, H, grad_image_ptr=grad, opacity_ptr=g["opacity"], sh_ptr=g["sh"])
        scene.adam_step(g, m, v, step=it, lr_sh_dc=0.01, lr_opacity=0.05, zero_grads=True)
        assert r.sync() == 0
    r.render(scene, cam, W, H, image.data_ptr())
    assert r.sync() == 0
    final = float(((image - target) ** 2).sum().item())
    print(f"descent: SSE {sse[0]:.6g} -> {final:.6g} after 40 steps (ratio {final / sse[0]:.4f})")
    assert sse[0] > 0 and final < sse[0]
    now = scene.download()
    frozen = [a for a in range(38) if a not in (3, 11, 12, 13)]
    assert same_bits(now[frozen], start[frozen])
