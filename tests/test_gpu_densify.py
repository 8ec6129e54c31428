"""Scene densification on the device (gsr_densify_accumulate, gsr_scene_densify,
gsr_densify_gather_planes, gsr_scene_reset_opacity; Scene.densify / Scene.reset_opacity,
densify_accumulate, densify_gather_planes): every output against the numpy twin
(tests/_densify_ref.py) bit for bit, and the closed loop render -> loss -> backward -> accumulate
-> step -> densify, after which the new block renders through the same context exactly as a
fresh upload of it does and as the oracle renders it."""
import numpy as np
import pytest

import _adam_ref
import _densify_ref as ref
from test_adam_ref import random_scene
from test_gpu_adam import ALL_LRS, PAD_BITS, read_block, upload_block, zeros_like_groups
from test_gpu_parity import CAMS, cam_for
from test_gpu_scene_ops import assert_header, dense_soa, dev, exact_renderer, frame, same_bits, special_bits

pytestmark = pytest.mark.gpu

C = ref.CHUNK                    # sources per workgroup of the expansion's kernels (kDensifyChunk)
GUARD = 64
SENT_SRC, SENT_KIND, SENT32 = -7, 0xEE, 0x5A5A5A5A
INF = float("inf")
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31


@pytest.fixture(scope="module")
def torch(gpu):
    import torch as t
    assert t.cuda.is_available()
    return t


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_chunk_constant(gpu):
    assert C == gpu.DENSIFY_CHUNK


# ---------------------------------------------------------------- 1. the statistic

def centre_planes(rng, n):
    """(2, n) gradients over twelve decades, with a share of Gaussians no pixel composited (+0 and
    -0 in both planes), of zeros in one plane only, and of NaN and infinities."""
    c = (10.0 ** rng.uniform(-9, 3, (2, n)) * rng.choice([-1.0, 1.0], (2, n))).astype(np.float32)
    kind = rng.integers(0, 10, n)
    c[:, kind == 0] = 0.0
    c[:, kind == 1] = -0.0
    c[0, kind == 2] = 0.0
    c[1, kind == 2] = -0.0
    c[0, kind == 3] = -0.0                         # one plane zero: still composited
    bad = np.flatnonzero(kind == 4)
    c[rng.integers(0, 2, bad.size), bad] = rng.choice(np.float32([np.nan, np.inf, -np.inf]), bad.size)
    return c


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 4097])
def test_accumulate(gpu, torch, n):
    rng = np.random.default_rng(n)
    W, H = 333, 217
    accum, seen, bad = np.zeros(n, np.float32), np.zeros(n, np.uint32), 0
    d_accum = torch.zeros(n + GUARD, dtype=torch.float32, device="cuda")
    d_seen = torch.zeros(n + GUARD, dtype=torch.int32, device="cuda")
    d_accum[n:] = 123.0
    d_seen[n:] = SENT_SRC
    d_bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    planted = [np.float32([[np.nan], [1.0]]), np.float32([[0.5], [-np.inf]])]
    for call in range(2):
        c = centre_planes(rng, n)
        c[:, :1] = planted[call]                                  # every size sees a non-finite entry
        accum, seen, b = ref.accumulate(c, W, H, accum, seen)
        bad += b
        gpu.densify_accumulate(dev(torch, c), n, W, H, d_accum, d_seen, bad_ptr=d_bad)
    torch.cuda.synchronize()
    got_a, got_s = d_accum.cpu().numpy(), d_seen.cpu().numpy()
    assert (got_a[n:] == 123.0).all() and (got_s[n:] == SENT_SRC).all(), "wrote past n"
    assert np.array_equal(bits(got_a[:n]), bits(accum)), np.flatnonzero(bits(got_a[:n]) != bits(accum))[:8]
    assert np.array_equal(got_s[:n].view(np.uint32), seen)
    assert int(d_bad.item()) == bad and bad >= 2
    if n >= 1000:
        assert 0 < (seen == 0).sum() and (seen == 2).sum() > n // 4
    # without a counter the same values arrive
    d2a, d2s = torch.zeros(n, dtype=torch.float32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    gpu.densify_accumulate(dev(torch, c), n, W, H, d2a, d2s)
    a1, s1, _ = ref.accumulate(c, W, H, np.zeros(n, np.float32), np.zeros(n, np.uint32))
    assert np.array_equal(bits(d2a.cpu().numpy()), bits(a1)) and np.array_equal(d2s.cpu().numpy().view(np.uint32), s1)


# ---------------------------------------------------------------- 2. the densify call

def scene_and_stats(narrays, n, rng):
    """A float32 scene with scales and opacities on both sides of the thresholds below, and a
    statistic with unseen Gaussians (seen == 0)."""
    soa = random_scene(narrays, n, rng).astype(np.float32)
    soa[3] = rng.uniform(0.0, 0.99, n)
    soa[4:7] = np.exp(rng.uniform(-5.0, -1.0, (3, n)))
    seen = rng.integers(0, 4, n).astype(np.uint32)
    accum = (rng.exponential(0.0004, n) * np.maximum(seen, 1)).astype(np.float32)
    return soa, accum, seen


MIX = dict(grad_threshold=0.0002, scale_split=0.1, min_opacity=0.05, prune_scale_max=0.3, split_shrink=1.6, seed=7)
SCENARIOS = {
    "kept": dict(MIX, grad_threshold=INF, min_opacity=0.0, prune_scale_max=INF),
    "pruned": dict(MIX, min_opacity=1.0),
    "cloned": dict(MIX, grad_threshold=0.0, scale_split=INF, min_opacity=0.0, prune_scale_max=INF),
    "split": dict(MIX, grad_threshold=0.0, scale_split=0.0, min_opacity=0.0, prune_scale_max=INF),
    "mixture": MIX,
}


def run_densify(gsr, torch, scene, d_accum, d_seen, cfg, lists=True):
    n = scene.n
    d_src = torch.full((2 * n + GUARD,), SENT_SRC, dtype=torch.int32, device="cuda") if lists else None
    d_kind = torch.full((2 * n + GUARD,), SENT_KIND, dtype=torch.uint8, device="cuda") if lists else None
    out, rep = scene.densify(d_accum, d_seen, src_ptr=d_src, kind_ptr=d_kind, **cfg)
    torch.cuda.synchronize()
    assert_header(gsr, torch, out, scene.narrays, rep["n_out"])
    return (out.download(), d_src.cpu().numpy() if lists else None, d_kind.cpu().numpy() if lists else None, rep)


def check_densify(gsr, torch, scene, soa, accum, seen, d_accum, d_seen, cfg, what):
    want, w_src, w_kind, w_rep = ref.densify(soa, accum, seen, cfg,
                                             lambda i, k: gsr.densify_normals(cfg["seed"], i, k))
    got, src, kind, rep = run_densify(gsr, torch, scene, d_accum, d_seen, cfg)
    m = w_rep["n_out"]
    assert rep == w_rep, what
    assert np.array_equal(src[:m], w_src) and (src[m:] == SENT_SRC).all(), what
    assert np.array_equal(kind[:m], w_kind) and (kind[m:] == SENT_KIND).all(), what
    diff = bits(got) != bits(want)
    assert got.shape == want.shape and not diff.any(), f"{what}: (array, j) {np.argwhere(diff)[:8].tolist()}"
    return got, src[:m], kind[:m], rep


@pytest.mark.parametrize("n", [1, 65, C - 1, C, C + 1, 2 * C + 1])
@pytest.mark.parametrize("narrays", [38, 49, 59])
def test_densify(gpu, torch, narrays, n):
    rng = np.random.default_rng(100 * narrays + n)
    soa, accum, seen = scene_and_stats(narrays, n, rng)
    scene = gpu.Scene.from_soa(soa)
    d_accum, d_seen = dev(torch, accum), dev(torch, seen)
    ident = np.arange(n, dtype=np.int32)

    got, src, kind, rep = check_densify(gpu, torch, scene, soa, accum, seen, d_accum, d_seen, SCENARIOS["kept"], "kept")
    assert rep == dict(n_out=n, kept=n, cloned=0, split=0, pruned=0)
    assert same_bits(got, soa) and np.array_equal(src, ident) and not kind.any()

    got, _, _, rep = check_densify(gpu, torch, scene, soa, accum, seen, d_accum, d_seen, SCENARIOS["pruned"], "pruned")
    assert rep["n_out"] == 0 and rep["pruned"] == n and got.shape == (narrays, 0)

    got, src, kind, rep = check_densify(gpu, torch, scene, soa, accum, seen, d_accum, d_seen, SCENARIOS["cloned"],
                                        "cloned")
    assert rep == dict(n_out=2 * n, kept=0, cloned=n, split=0, pruned=0)
    assert np.array_equal(src, ident.repeat(2)) and np.array_equal(kind, np.tile(np.uint8([0, 1]), n))
    assert same_bits(got[:, 0::2], soa) and same_bits(got[:, 1::2], soa)

    got, src, kind, rep = check_densify(gpu, torch, scene, soa, accum, seen, d_accum, d_seen, SCENARIOS["split"], "split")
    assert rep == dict(n_out=2 * n, kept=0, cloned=0, split=n, pruned=0)
    assert np.array_equal(src, ident.repeat(2)) and np.array_equal(kind, np.tile(np.uint8([2, 3]), n))
    rest = [3] + list(range(7, narrays))
    assert same_bits(got[rest], soa[rest][:, src]) and not (bits(got[4:7]) == bits(soa[4:7][:, src])).any()


@pytest.mark.parametrize("n", [1, 65, C - 1, C, C + 1, 2 * C + 1])
@pytest.mark.parametrize("narrays", [38, 49, 59])
def test_densify_mixture(gpu, torch, narrays, n):
    """Every fate in one scene (from n = 65 on), with a NaN accumulator, unseen Gaussians, and
    kept Gaussians that carry a NaN opacity and a NaN scale component (compared, never computed
    with); two runs; another seed; no lists."""
    rng = np.random.default_rng(200 * narrays + n)
    soa, accum, seen = scene_and_stats(narrays, n, rng)
    accum[rng.integers(0, n)] = np.nan                   # avg >= threshold is false: never hot
    q = rng.integers(0, n, 2)
    seen[q] = 0
    soa[3, q[0]] = np.nan                                # NaN < min_opacity is false: not pruned
    soa[4, q[1]], soa[5:7, q[1]] = np.nan, 0.01          # fmaxf skips the NaN
    scene = gpu.Scene.from_soa(soa)
    d_accum, d_seen = dev(torch, accum), dev(torch, seen)
    got, src, kind, rep = check_densify(gpu, torch, scene, soa, accum, seen, d_accum, d_seen, MIX, "mixture")
    if n >= 65:
        assert min(rep["kept"], rep["cloned"], rep["split"], rep["pruned"]) > 0, rep
        assert (seen == 0).any()
    assert rep["kept"] + rep["cloned"] + rep["split"] + rep["pruned"] == n

    again = run_densify(gpu, torch, scene, d_accum, d_seen, MIX)
    assert same_bits(again[0], got) and np.array_equal(again[1][:rep["n_out"]], src) and again[3] == rep
    assert np.array_equal(again[2][:rep["n_out"]], kind)

    other = run_densify(gpu, torch, scene, d_accum, d_seen, dict(MIX, seed=8))
    assert other[3] == rep and np.array_equal(other[1][:rep["n_out"]], src)
    moved = bits(other[0]) != bits(got)
    kids = kind >= 2
    assert not moved[3:].any() and not moved[:, ~kids].any()
    if kids.any():
        assert moved[0:3][:, kids].any(axis=0).all()

    nolists = run_densify(gpu, torch, scene, d_accum, d_seen, MIX, lists=False)
    assert same_bits(nolists[0], got) and nolists[3] == rep


def test_densify_of_nothing_and_mismatch(gpu, torch):
    empty = gpu.Scene.from_soa(np.zeros((38, 0), np.float32))
    out, rep = empty.densify(None, None, **MIX)
    assert rep == dict(n_out=0, kept=0, cloned=0, split=0, pruned=0) and out.n == 0
    assert_header(gpu, torch, out, 38, 0)
    soa, accum, seen = scene_and_stats(38, 100, np.random.default_rng(1))
    scene = gpu.Scene.from_soa(soa)
    wrong = gpu.Scene(scene.ptr, 101, owned=False, narrays=38)
    with pytest.raises(gpu.GsrError, match="block holds"):
        wrong.densify(dev(torch, accum), dev(torch, seen), **MIX)


# ---------------------------------------------------------------- 3. the masked moment gather

@pytest.mark.parametrize("nplanes", [1, 8, 9, 27])
def test_gather_planes(gpu, torch, nplanes):
    n = 500
    rng = np.random.default_rng(nplanes)
    src = rng.integers(0, 2 ** 32, (nplanes, n + 3), dtype=np.uint64).astype(np.uint32)
    sp = special_bits(np.uint32)
    src[:, :sp.size] = sp
    d_src = dev(torch, src)
    for m in (1, 63, 64, 65, 777):
        idx = np.sort(rng.integers(0, n, m)).astype(np.int32)
        idx[:min(m, sp.size)] = np.arange(min(m, sp.size))
        kind = rng.choice(np.uint8([0, 0, 1, 2, 3]), m)
        kind[:min(m, sp.size)] = 0                                  # the special values are read
        d_dst = torch.full((nplanes, m + 5), SENT32, dtype=torch.int32, device="cuda")
        gpu.densify_gather_planes(d_dst, m + 5, d_src, n + 3, nplanes, n, dev(torch, idx), dev(torch, kind), m)
        torch.cuda.synchronize()
        got = d_dst.cpu().numpy().view(np.uint32)
        want, bad = ref.gather_planes(src.view(np.float32)[:, :n], idx, kind)
        assert bad == 0
        assert np.array_equal(got[:, :m], bits(want)), (nplanes, m)
        assert np.array_equal(got[:, :m][:, kind == 0], src[:, idx[kind == 0]])       # survivors: bit for bit
        assert not got[:, :m][:, kind != 0].any()                                    # new Gaussians: exactly +0
        assert (got[:, m:] == SENT32).all()


def test_gather_planes_bad_indices(gpu, torch):
    """An out-of-range index that is read (kind 0) is clamped and counted; one that is not read
    (kind != 0) forms no address and counts nothing."""
    n, m, nplanes = 300, 700, 5
    rng = np.random.default_rng(3)
    src = rng.normal(0, 1, (nplanes, n)).astype(np.float32)
    idx = rng.integers(0, n, m).astype(np.int64)
    where = rng.choice(m, 80, replace=False)
    idx[where] = np.tile([-1, n, INT32_MAX, INT32_MIN], 20)
    kind = rng.choice(np.uint8([0, 1, 3]), m)
    kind[where[:40]] = 0
    kind[[0, 63, 64, m - 1]] = 0
    idx[[0, 63, 64, m - 1]] = [-1, INT32_MIN, n, INT32_MAX]
    want, bad = ref.gather_planes(src, idx, kind)
    assert 44 <= bad < 84
    d_bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_dst = torch.full((nplanes, m), SENT32, dtype=torch.int32, device="cuda")
    gpu.densify_gather_planes(d_dst, m, dev(torch, src), n, nplanes, n, dev(torch, idx.astype(np.int32)),
                              dev(torch, kind), m, bad_ptr=d_bad)
    assert int(d_bad.item()) == bad
    assert np.array_equal(d_dst.cpu().numpy().view(np.uint32), bits(want))


# ---------------------------------------------------------------- 4. the opacity reset

@pytest.mark.parametrize("narrays,n", [(38, 1), (38, 65), (49, 1000), (59, 4097)])
def test_reset_opacity(gpu, torch, narrays, n):
    rng = np.random.default_rng(narrays + n)
    soa = random_scene(narrays, n, rng).astype(np.float32)
    soa[3] = rng.uniform(0.0, 1.0, n)
    soa[3, 0] = 0.004 if n > 1 else 0.5
    soa[3, n // 2] = np.nan
    cap = 0.01
    want = ref.reset_opacity(soa, cap)
    assert n == 1 or ((bits(want[3]) != bits(soa[3])).any() and (bits(want[3]) == bits(soa[3])).any())
    scene = upload_block(gpu, torch, soa)
    before = read_block(gpu, torch, scene)
    moments = [torch.full((n + GUARD,), 3.5, dtype=torch.float32, device="cuda") for _ in range(2)]
    scene.reset_opacity(cap, moments[0], moments[1])
    torch.cuda.synchronize()
    after = read_block(gpu, torch, scene)
    assert np.array_equal(after[3, :n], bits(want[3])) and (after[3, n:] == PAD_BITS).all()
    rest = [a for a in range(narrays) if a != 3]
    assert np.array_equal(after[rest], before[rest])                 # padding included
    assert_header(gpu, torch, scene, narrays, n)
    for t in moments:
        h = t.cpu().numpy()
        assert not bits(h[:n]).any() and (h[n:] == 3.5).all()
    # without moment planes, and a second reset changes nothing
    scene.reset_opacity(cap)
    torch.cuda.synchronize()
    assert np.array_equal(read_block(gpu, torch, scene), after)


# ---------------------------------------------------------------- 5. the closed loop

W = H = 64


def test_training_loop_with_densify(gpu, orc, torch):
    """Two iterations of render, image_loss, render_backward_scene with a caller scratch,
    densify_accumulate and adam_step on the 600-Gaussian dense scene at 64 x 64; then a densify
    with thresholds between the statistic's and the scene's own quantiles, so that every fate
    occurs.  No claim about the loss value is tested."""
    soa = dense_soa()
    n = soa.shape[1]
    scene = gpu.Scene.from_soa(soa)
    cam = cam_for(gpu, W, H, **CAMS[0])
    r = exact_renderer(gpu, diagnostics=True)
    rng = np.random.default_rng(12)
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
    assert frame(gpu, torch, r, scene, cam, W, H) is not None       # grows the context's buffers

    def backward(sc, grads, rec):
        for _ in range(3):
            r.render(sc, cam, W, H, image.data_ptr())
            gpu.image_loss(image, target, W, H, grad_ptr=grad_image, scratch_ptr=loss_scratch,
                           scratch_bytes=scratch_bytes)
            for t in grads.values():
                t.zero_()
            r.render_backward_scene(sc, cam, W, H, grad_image_ptr=grad_image, scratch_ptr=rec,
                                    **{k + "_ptr": t for k, t in grads.items()})
            if r.sync() == 0:
                return
        raise AssertionError("frame still incomplete after three renders")

    for it in (1, 2):
        backward(scene, g, record)
        gpu.densify_accumulate(record[8 * n:], n, W, H, d_accum, d_seen, bad_ptr=d_bad)
        scene.adam_step(g, m, v, step=it, bad_ptr=d_bad, **ALL_LRS)
    torch.cuda.synchronize()
    assert int(d_bad.item()) == 0
    accum, seen = d_accum.cpu().numpy(), d_seen.cpu().numpy().view(np.uint32)
    assert (seen == 2).sum() > 100 and (seen == 0).sum() > 0
    now = scene.download()
    avg = accum[seen > 0] / seen[seen > 0]
    cfg = dict(grad_threshold=float(np.median(avg)), scale_split=float(np.median(now[4:7].max(axis=0))),
               min_opacity=float(np.quantile(now[3], 0.1)), prune_scale_max=INF, split_shrink=1.6, seed=2024)

    d_src = torch.full((2 * n,), SENT_SRC, dtype=torch.int32, device="cuda")
    d_kind = torch.full((2 * n,), SENT_KIND, dtype=torch.uint8, device="cuda")
    grown, rep = scene.densify(d_accum, d_seen, src_ptr=d_src, kind_ptr=d_kind, **cfg)
    print("densify report:", rep)
    assert min(rep["kept"], rep["cloned"], rep["split"], rep["pruned"]) > 10, rep
    n2 = grown.n
    want = ref.densify(now, accum, seen, cfg, lambda i, k: gpu.densify_normals(cfg["seed"], i, k))
    soa2 = grown.download()
    assert same_bits(soa2, want[0]) and rep == want[3]

    # the new block through the SAME context, against a fresh upload of its download and the oracle
    got = frame(gpu, torch, r, grown, cam, W, H)
    takes = r.take_map(W, H)
    r2 = exact_renderer(gpu, diagnostics=True)
    fresh = frame(gpu, torch, r2, gpu.Scene.from_soa(soa2), cam, W, H)
    assert same_bits(got, fresh) and np.array_equal(takes, r2.take_map(W, H))
    assert same_bits(got, orc.render(soa2, cam, W, H, 3.0))
    assert (got != 0).sum() > 1000

    # the moments cut over: survivors keep theirs, new Gaussians start at zero; the step runs
    P = _adam_ref.planes_of(38)
    g2 = zeros_like_groups(torch, n2)
    m2, v2 = ({k: torch.full((P[k] * n2,), float("nan"), dtype=torch.float32, device="cuda") for k in mom}
              for mom in (m, v))
    for old, new in ((m, m2), (v, v2)):
        for k in old:
            gpu.densify_gather_planes(new[k], n2, old[k], n, P[k], n, d_src, d_kind, n2, bad_ptr=d_bad)
    src, kind = want[1], want[2]
    for k in m:
        h_old, h_new = m[k].cpu().numpy().reshape(P[k], n), m2[k].cpu().numpy().reshape(P[k], n2)
        assert same_bits(h_new[:, kind == 0], h_old[:, src[kind == 0]]) and not bits(h_new[:, kind != 0]).any()
        assert h_old.any()
    record2 = torch.zeros(10 * n2, dtype=torch.float32, device="cuda")
    backward(grown, g2, record2)
    grown.adam_step(g2, m2, v2, step=3, bad_ptr=d_bad, **ALL_LRS)
    torch.cuda.synchronize()
    assert int(d_bad.item()) == 0
    assert (grown.download() != soa2).mean() > 0.1
    # and the statistic starts over on the new scene
    d_accum2 = torch.zeros(n2, dtype=torch.float32, device="cuda")
    d_seen2 = torch.zeros(n2, dtype=torch.int32, device="cuda")
    gpu.densify_accumulate(record2[8 * n2:], n2, W, H, d_accum2, d_seen2, bad_ptr=d_bad)
    assert int(d_bad.item()) == 0 and int(d_seen2.sum().item()) > 100
