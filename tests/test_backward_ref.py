"""The yardstick of gsr_render_backward's GPU tests (tests/_backward_ref.py), checked on the
CPU: against the unmodified oracle, against its own finite differences, for the share of
ambiguous pixels, and in float32 (E32, from which the GPU tolerance is taken)."""
import numpy as np
import pytest

import _backward_ref as br
from test_gpu_backward import E32


@pytest.fixture(scope="module")
def ref(gsr, orc, tmp_path_factory):
    return lambda case, g=(5, False, True, True): br.reference(gsr, orc, tmp_path_factory, case, g)


@pytest.mark.parametrize("case", sorted(br.CASES))
def test_reference_forward_is_the_oracles(gsr, orc, ref, case):
    """The forward image within 1e-6 of orc.render, and the take counts equal to the low words
    of orc.render_takes at every unmasked pixel."""
    c = br.CASES[case]
    r = ref(case)
    img, tk = orc.render_takes(r["soa"], br.camera(gsr, case), c["W"], c["H"], c.get("k", 3.0),
                               tiling=c.get("tiling"))
    um = ~r["mask"]
    if "region" in c:     # only these pixels were evaluated
        x0, x1, y0, y1 = c["region"]
        um[:y0], um[y1 + 1:], um[:, :x0], um[:, x1 + 1:] = False, False, False, False
    err = float(np.abs(img.astype(np.float64) - r["image"])[:, um].max())
    print(case, "image error", err, "takes up to", int(r["takes"].max()))
    # (the overflow case: 1700 takes per pixel, where the float32 oracle itself is 1.6e-6 off)
    assert err <= (4e-6 if case == "overflow" else 1e-6)
    assert np.array_equal((tk & np.uint64(0xFFFFFFFF)).astype(np.int64)[um], r["takes"][um])
    assert r["takes"].sum() > 500


@pytest.mark.parametrize("case", sorted(br.CASES))
def test_mask_share_within_cap(ref, case):
    r = ref(case)
    share = br.mask_share(r)
    print(case, "masked", int(r["mask"].sum()), "share", share)
    if case == "overflow":      # outside the condition by construction: _backward_ref.CASES
        assert (~r["mask"] & (r["takes"] > 0)).sum() >= 80
        return
    assert share <= br.MASK_SHARE_CAP


def test_reference_against_finite_differences(ref):
    """32 random (Gaussian, component) pairs: the analytic gradient agrees with a central
    difference (relative step 1e-6, inside the mask's margins) to 1e-6 of its scale."""
    rng = np.random.default_rng(31)
    worst = 0.0
    for case, g, count in (("dense", (5, False, True, True), 20), ("sparse_a", (8, False, True, True), 12)):
        c = br.CASES[case]
        r = ref(case, g)
        taken = np.flatnonzero(r["A_opacity"][0] > 0)
        assert len(taken) > 50
        for _ in range(count):
            while True:     # (a one-pixel-wide splat has no dx dy: A = 0, nothing to compare)
                i = int(rng.choice(taken))
                kind, comps = br.KINDS[int(rng.integers(4))]
                comp = int(rng.integers(comps))
                if r["A_" + kind][comp, i] > 0:
                    break
            fd = br.finite_difference(r["rec"], c["W"], c["H"], r["g_image"], r["g_alpha"], kind, comp, i)
            an, A = float(r[kind][comp, i]), float(r["A_" + kind][comp, i])
            print(case, i, kind, comp, "analytic", an, "fd", fd, "A", A)
            assert A > 0
            worst = max(worst, abs(fd - an) / A)
            assert abs(fd - an) <= 1e-6 * A
    print("worst |fd - analytic| / A", worst)


def test_float32_error_is_e32(gsr, orc, ref):
    """The reference evaluated in float32 against itself in float64, over every run the GPU
    tests compare: the largest error / A is what single precision alone costs.  The GPU tests'
    constant E32 is that figure rounded up, and outside the mask float32 takes the float64
    decisions."""
    worst = 0.0
    for case, g in br.RUNS:
        c = br.CASES[case]
        r = ref(case, g)
        r32 = br.evaluate(r["rec"], c["W"], c["H"], r["g_image"], r["g_alpha"], c.get("tiling"), dtype=np.float32,
                          zero_masked=False, region=c.get("region"))
        um = ~r["mask"]
        assert np.array_equal(r32["takes"][um], r["takes"][um])
        e, clean = br.error_over_scale(r32, r)
        print(case, g, "E32", e)
        assert clean
        worst = max(worst, e)
    print("E32 over all runs", worst)
    assert E32 / 2 <= worst <= E32
