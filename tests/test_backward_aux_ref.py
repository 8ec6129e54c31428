"""The yardstick of gsr_render_backward_aux's GPU tests (tests/_backward_aux_ref.py), checked on
the CPU: its depth and feature planes against the unmodified oracle, its gradients against its
own finite differences, the share of ambiguous pixels per run, and in float32 (E32_AUX, from
which the GPU tolerance is taken).  These tests check the yardstick, not the feature: but for
the import of the GPU test's constant they need nothing the library gained with it."""
import numpy as np
import pytest

import _backward_aux_ref as bar
import _backward_ref as br
from test_gpu_backward_aux import E32_AUX

SH_C0 = 0.28209479177387814
F_DC, F_REST = slice(11, 14), slice(14, 38)


@pytest.fixture(scope="module")
def ref(gsr, orc, tmp_path_factory):
    return lambda case, sp=bar.ALL4, **kw: bar.reference(gsr, orc, tmp_path_factory, case, sp, **kw)


@pytest.mark.parametrize("case", ["dense", "dense_partial", "sparse_a", "4d", "tilted_k8"])
def test_reference_planes_are_the_oracles(gsr, orc, tmp_path_factory, case):
    """tests/test_gpu_aux.py's recolouring: a copy of the scene with f_rest zeroed and chosen f_dc
    gives any per-Gaussian colour in [0, 1] over the same geometry, and every aux channel
    accumulates like a colour.  Features: the oracle's preprocessed colours of a randomly
    recoloured scene, as the reference's feature values, give that scene's image.  Depth: the
    recolouring whose colour is z / s (s twice the largest visible z) gives depth / s.  The
    tolerance is tests/test_backward_ref.py's for image and alpha, 1e-6."""
    c = br.CASES[case]
    W, H, k, tiling = c["W"], c["H"], c.get("k", 3.0), c.get("tiling")
    soa = br.scenes(gsr, orc, tmp_path_factory)[c["scene"]]
    if "time" in c:
        soa = orc.temporal(soa, c["time"])
    cam = br.camera(gsr, case)
    n = soa.shape[1]
    s2 = soa.copy()
    s2[F_REST] = 0.0
    s2[F_DC] = np.random.default_rng(7).uniform(-3.0, 3.0, (3, n)).astype(np.float32)
    feat = np.ascontiguousarray(orc.preprocess(s2, cam, W, H, k)["color"].T)     # (3, n) in [0, 1]
    rec = bar.records(orc, soa, cam, W, H, k, feat)
    z = rec["z"][0]
    vis = rec["order"]
    scale = 2.0 * float(z[vis].max())
    assert z[vis].min() > 0
    s3 = soa.copy()
    s3[F_REST] = 0.0
    s3[F_DC] = 0.0
    s3[11] = ((np.where(z > 0, z, 0.0) / scale - 0.5) / SH_C0).astype(np.float32)
    zc = orc.preprocess(s3, cam, W, H, k)["color"][:, 0].astype(np.float64)      # the colours composited
    assert np.abs(zc[vis] - z[vis] / scale).max() <= 2e-7
    r = bar.evaluate(rec, W, H, tiling=tiling, grads=False)
    um = ~r["mask"]
    want_f = orc.render(s2, cam, W, H, k, tiling=tiling).astype(np.float64)
    want_z = orc.render(s3, cam, W, H, k, tiling=tiling)[0].astype(np.float64)
    err_f = float(np.abs(want_f - r["feat_planes"])[:, um].max())
    err_z = float(np.abs(want_z - r["depth"] / scale)[um].max())
    print(case, "feature planes", err_f, "depth / s", err_z, "s", scale)
    assert r["takes"].sum() > 500 and (r["depth"] > 0).sum() > 100
    assert err_f <= 1e-6 and err_z <= 1e-6


@pytest.mark.parametrize("case,sp", bar.RUNS_AUX)
def test_mask_share_within_cap(ref, case, sp):
    r = ref(case, sp)
    share = br.mask_share(r)
    print(case, "masked", int(r["mask"].sum()), "share", share)
    if case == "overflow":      # outside the condition by construction: _backward_ref.CASES
        assert (~r["mask"] & (r["takes"] > 0)).sum() >= 80
        return
    assert share <= bar.MASK_SHARE_CAP


# (case, upstream, kinds differenced, samples): z and the features under every upstream; the
# geometry under depth-only and feature-only upstream, where u is made of the new terms alone
FD_RUNS = [
    ("dense", bar.ALL4, ("z", "feat"), 10),
    ("sparse_a", bar.ALL8, ("z", "feat"), 6),
    ("dense", bar.spec(20, image=False, alpha=False), ("opacity", "conic", "center", "z"), 10),
    ("dense", bar.spec(22, image=False, alpha=False, depth=False, nfeat=1), ("opacity", "conic", "center", "feat"), 10),
]


@pytest.mark.parametrize("case,sp,names,count", FD_RUNS)
def test_reference_against_finite_differences(ref, case, sp, names, count):
    """Random (Gaussian, kind, component) triples: the analytic gradient agrees with a central
    difference (relative step 1e-6, inside the mask's margins) to 1e-6 of its scale."""
    rng = np.random.default_rng(41 + sp[0])
    c = br.CASES[case]
    r = ref(case, sp)
    comps = dict(bar.kinds(r["nfeat"]))
    taken = np.flatnonzero(r["count"] > 0)
    assert len(taken) > 50
    worst = 0.0
    for _ in range(count):
        while True:     # (a one-pixel-wide splat has no dx dy: A = 0, nothing to compare)
            i = int(rng.choice(taken))
            kind = names[int(rng.integers(len(names)))]
            comp = int(rng.integers(comps[kind]))
            if r["A_" + kind][comp, i] > 0:
                break
        fd = bar.finite_difference(r["rec"], c["W"], c["H"], bar.upstream_of(r), kind, comp, i)
        an, A = float(r[kind][comp, i]), float(r["A_" + kind][comp, i])
        print(case, i, kind, comp, "analytic", an, "fd", fd, "A", A)
        worst = max(worst, abs(fd - an) / A)
        assert abs(fd - an) <= 1e-6 * A
    print("worst |fd - analytic| / A", worst)


def test_float32_error_is_e32_aux(ref):
    """The reference evaluated in float32 against itself in float64, over every run the GPU
    tests compare and every kind of output, z and the features included: the largest error / A
    is what single precision alone costs.  The GPU tests' constant E32_AUX is that figure
    rounded up, and outside the mask float32 takes the float64 decisions."""
    worst = 0.0
    for case, sp in bar.RUNS_AUX:
        c = br.CASES[case]
        r = ref(case, sp)
        r32 = bar.evaluate(r["rec"], c["W"], c["H"], *bar.upstream_of(r), tiling=c.get("tiling"), dtype=np.float32,
                           zero_masked=False, region=c.get("region"))
        um = ~r["mask"]
        assert np.array_equal(r32["takes"][um], r["takes"][um])
        e, clean = bar.error_over_scale(r32, r, r["nfeat"])
        print(case, sp, "E32", e)
        assert clean
        worst = max(worst, e)
    print("E32_AUX over all runs", worst)
    assert E32_AUX / 2 <= worst <= E32_AUX
