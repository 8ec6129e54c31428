"""The yardstick of gsr_project_backward's GPU tests (tests/_project_ref.py), checked on the
CPU: its forward against the unmodified oracle's preprocess, its valid set against the
oracle's status, its autograd gradients against central differences of its own forward, the
share of Gaussians it leaves out, and itself in float32 (E32, from which the GPU tolerance is
taken)."""
import numpy as np
import pytest
import torch

import _project_ref as pr
from test_gpu_project_backward import E32

# The largest distance between the restatement in float32 and in float64 over every case and
# status-2 Gaussian, per record field (measured: the test asserts each constant against its
# measurement).  The oracle computes in float32 in another operation order, so it may stand
# 8 x as far from the float64 restatement.
# Measured: colour 2.15e-7, opacity 2.55e-7 (the 4D case's exp), conic 1.68e-6, view 1.04e-7,
# ndc 1.79e-7.
F32_DISTANCE = {"color": 2.5e-7, "opacity": 3.0e-7, "conic": 2.0e-6, "view": 1.2e-7, "ndc": 2.0e-7}


@pytest.fixture(scope="module")
def ref(gsr, tmp_path_factory):
    return lambda case: pr.reference(gsr, tmp_path_factory, case)


def oracle_splats(gsr, orc, r, case):
    c = pr.CASES[case]
    soa, cam = r["soa"], pr.camera(gsr, case)
    if soa.shape[0] == 49:
        return orc.preprocess(orc.temporal(soa, c["time"]), cam, c["W"], c["H"], 3.0)
    if soa.shape[0] == 59:
        with orc.sh3_mode():
            return orc.preprocess(soa, cam, c["W"], c["H"], 3.0)
    return orc.preprocess(soa, cam, c["W"], c["H"], 3.0)


def distances(a, b, sel):
    """Per record field, the largest distance between two forwards over the Gaussians sel:
    colour, opacity and ndc absolute; view relative to the largest |coordinate| of the point (at
    least 1); conic entries relative to the largest |entry| of the Gaussian."""
    d = {}
    for k in ("color", "opacity", "ndc"):
        d[k] = float(np.abs(np.asarray(a[k], np.float64) - b[k])[..., sel].max())
    vs = np.maximum(np.abs(b["view"][:3]).max(0), 1.0)
    d["view"] = float((np.abs(np.asarray(a["view"][:3], np.float64) - b["view"][:3]) / vs)[:, sel].max())
    cs = np.abs(b["conic"]).max(0)
    d["conic"] = float((np.abs(np.asarray(a["conic"], np.float64) - b["conic"]) / cs)[:, sel].max())
    return d


def test_forward_is_the_oracles(gsr, orc, ref):
    worst32 = dict.fromkeys(F32_DISTANCE, 0.0)
    for case in pr.CASES:
        c = pr.CASES[case]
        r = ref(case)
        spl = oracle_splats(gsr, orc, r, case)
        vis = spl["status"] == 2
        assert vis.sum() >= (1 if case == "n1" else 50) and r["valid"][vis].all()
        r32 = pr.evaluate(r["soa"], r["camv"], c["W"], c["H"], c.get("time", 0.0), dtype=torch.float32,
                          valid=r["valid"])
        d32 = distances(r32, r, vis)
        orc_fields = {"color": spl["color"].T, "opacity": spl["opacity"], "ndc": spl["ndc"].T, "view": spl["view"].T,
                      "conic": spl["inv_covar"].T}
        dor = distances(orc_fields, r, vis)
        print(case, "float32 restatement", d32, "oracle", dor)
        for k in F32_DISTANCE:
            worst32[k] = max(worst32[k], d32[k])
            assert dor[k] <= 8 * F32_DISTANCE[k], (case, k, dor[k])
        # the record's centre is the rounded one
        cen = r["center"][:, vis]
        frac = cen - np.floor(cen)
        clear = (np.abs(frac - 0.5) > 1e-3).all(0)
        px = np.stack([spl["px_x"][vis], spl["px_y"][vis]])
        assert (~clear).sum() <= max(2, 0.01 * clear.size)      # two rings of 2e-3 per pixel: 0.4 % expected
        assert np.array_equal(np.floor(cen + 0.5)[:, clear].astype(np.int64), px[:, clear].astype(np.int64))
    print("float32 restatement, worst", worst32)
    for k, v in F32_DISTANCE.items():
        assert v / 2 <= worst32[k] <= v, (k, worst32[k])


@pytest.mark.parametrize("case", sorted(pr.CASES))
def test_valid_set_and_share_left_out(gsr, orc, ref, case):
    """Outside the ambiguity margin the valid set holds every status-2 Gaussian and no status-0
    one; at most 2 % of the valid Gaussians are left out of the comparison."""
    r = ref(case)
    spl = oracle_splats(gsr, orc, r, case)
    sure = ~r["ambiguous"]
    assert r["valid"][(spl["status"] == 2) & sure].all()
    assert not r["valid"][(spl["status"] == 0) & sure].any()
    share = pr.ambiguous_share(r)
    print(case, "valid", int(r["valid"].sum()), "status", np.bincount(spl["status"], minlength=3), "ambiguous",
          int(r["ambiguous"].sum()), "share", share, "temporal underflow", int(r["underflow"].sum()))
    assert share <= pr.AMBIGUOUS_SHARE_CAP
    assert not r["upstream"][:, r["ambiguous"]].any()
    if case == "sparse_in":
        assert (spl["status"] == 0).sum() >= 100 and (~r["valid"]).sum() >= 100
    if case in ("sparse_a", "sparse_b"):
        assert (spl["status"] == 1).sum() >= 100     # off screen: valid here, never composited in a frame
    if case == "4d":
        assert 0 < r["underflow"].sum() < r["valid"].sum() / 4


@pytest.mark.parametrize("case", ["dense", "rot", "sparse_a", "sparse_in", "sh3", "4d"])
def test_autograd_against_central_differences(ref, case):
    """20 (Gaussian, array) pairs per output group: the autograd gradient agrees with a central
    difference of the float64 forward (relative step 1e-6) to 1e-6 of the group's scale: the
    difference's own error is about eps / step = 2e-10 of the record's magnitude over the
    array's, and step^2 = 1e-12 of the third derivative's."""
    c = pr.CASES[case]
    r = ref(case)
    rng = np.random.default_rng(17)
    live = np.flatnonzero(r["valid"] & r["upstream"].any(0))
    worst = 0.0
    for name, rows in pr.groups(r["soa"].shape[0]).items():
        for _ in range(20):
            while True:
                i, j = int(rng.choice(live)), int(rng.integers(rows.start, rows.stop))
                if r["A"][j, i] > 0:
                    break
            fd = pr.central_difference(r["soa"], r["camv"], c["W"], c["H"], c.get("time", 0.0), r["upstream"], j, i)
            err = abs(fd - r["grad"][j, i]) / r["A"][j, i]
            worst = max(worst, err)
            assert err <= 1e-6, (case, name, j, i, fd, r["grad"][j, i], r["A"][j, i])
    print(case, "worst |fd - autograd| / A", worst)


def test_float32_error_is_e32(ref):
    """The reference evaluated in float32 torch against itself in float64, over every case the
    GPU test compares: the largest error / A is what single precision alone costs.  The GPU
    tests' constant E32 is that figure rounded up."""
    worst = 0.0
    for case in pr.CASES:
        c = pr.CASES[case]
        r = ref(case)
        r32 = pr.evaluate(r["soa"], r["camv"], c["W"], c["H"], c.get("time", 0.0), upstream=r["upstream"],
                          dtype=torch.float32, valid=r["valid"])
        e = pr.error_over_scale(r32["grad"], r["grad"], r["A"])
        per = {g: pr.error_over_scale(r32["grad"][rows], r["grad"][rows], r["A"][rows])
               for g, rows in pr.groups(r["soa"].shape[0]).items()}
        print(case, "E32", e, per)
        assert not r32["grad"][r["A"] == 0].any()
        worst = max(worst, e)
    print("E32 over all cases", worst)
    assert E32 / 2 <= worst <= E32
