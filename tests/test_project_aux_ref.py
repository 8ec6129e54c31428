"""The yardstick of gsr_project_backward_aux's GPU tests (tests/_project_aux_ref.py), checked on
the CPU: the eleventh record component against the unmodified oracle's view z, the d_z gradient
against central differences, and the reference in float32 (E32_AUX, from which the GPU tolerance
is taken)."""
import numpy as np
import pytest
import torch

import _project_aux_ref as par
import _project_ref as pr
from test_gpu_project_backward_aux import E32_AUX


@pytest.fixture(scope="module")
def ref(gsr, tmp_path_factory):
    return lambda case, mode: par.reference(gsr, tmp_path_factory, case, mode)


@pytest.mark.parametrize("case", ["rot", "4d"])
def test_minus_z_is_the_oracles(gsr, orc, ref, case):
    """Record component 10 of the float64 restatement against the oracle's float32 -view z, within
    8 x the 1.2e-7 tests/test_project_ref.py measures for the view position (relative to |view|)."""
    c = pr.CASES[case]
    r = ref(case, "z")
    soa = r["soa"]
    spl = orc.preprocess(orc.temporal(soa, c["time"]) if soa.shape[0] == 49 else soa, pr.camera(gsr, case),
                         c["W"], c["H"], 3.0)
    vis = (spl["status"] == 2) & r["valid"]
    assert vis.sum() > 100
    with torch.no_grad():
        f = pr.forward(torch.from_numpy(soa.astype(np.float64)), r["camv"], c["W"], c["H"], c.get("time", 0.0))
    z = par.record(f).numpy()[10]
    norm = np.sqrt((f["view"].numpy()[:3] ** 2).sum(0))
    err = np.abs(z - (-spl["view"][:, 2].astype(np.float64)))[vis] / norm[vis]
    print(case, "-Z against the oracle", float(err.max()))
    assert (z[vis] > 0).all() and err.max() <= 8 * 1.2e-7


@pytest.mark.parametrize("case", ["rot", "4d"])
def test_dz_against_central_differences(ref, case):
    """d_z alone: position (and, 4D, trbf_center and the motion arrays) against a central
    difference, to 1e-6 of the group's scale."""
    c = pr.CASES[case]
    r = ref(case, "z")
    rng = np.random.default_rng(77)
    live = np.flatnonzero(r["valid"] & r["upstream"].any(0))
    rows = [0, 1, 2] + ([38, 40, 43, 48] if r["soa"].shape[0] == 49 else [])
    worst = 0.0
    for _ in range(12):
        i, j = int(rng.choice(live)), int(rng.choice(rows))
        fd = par.central_difference(r["soa"], r["camv"], c["W"], c["H"], c.get("time", 0.0), r["upstream"], j, i)
        an, A = float(r["grad"][j, i]), float(r["A"][j, i])
        print(case, i, j, "analytic", an, "fd", fd, "A", A)
        assert A > 0 and abs(fd - an) <= 1e-6 * A
        worst = max(worst, abs(fd - an) / A)
    print("worst", worst)
    # nothing but the position and the temporal arrays depends on Z
    other = np.ones(r["soa"].shape[0], bool)
    other[0:3] = False
    other[38:] = False
    assert not r["grad"][other].any()


def test_float32_error_is_e32_aux(ref):
    """The reference in float32 torch against itself in float64 over every run the GPU tests
    compare; the GPU tests' constant E32_AUX is that figure rounded up."""
    worst = 0.0
    for case, mode in par.RUNS:
        c = pr.CASES[case]
        r = ref(case, mode)
        r32 = par.evaluate(r["soa"], r["camv"], c["W"], c["H"], c.get("time", 0.0), upstream=r["upstream"],
                           dtype=torch.float32, valid=r["valid"])
        e = pr.error_over_scale(r32["grad"], r["grad"], r["A"])
        print(case, mode, "E32", e)
        assert not r32["grad"][r["A"] == 0].any()
        worst = max(worst, e)
    print("E32_AUX over all runs", worst)
    assert E32_AUX / 2 <= worst <= E32_AUX
