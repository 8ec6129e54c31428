"""Preconditions of tests/test_gpu_temporal.py, on the CPU: the scenes of
tests/_temporal_scenes.py reach the 4D preprocess's temporal cull at its boundary and its
temporal arithmetic at its edge values.  Everything here is computed from the oracle alone
(orc.temporal, orc.preprocess, orc.render_takes), never from the kernels.  What a case reaches
depends on its seed, so every floor is asserted per case, with the measured count printed
beside it.

The last test is the cull's proof checked independently of the kernel: a visible Gaussian
whose opacity at t is below 0.9e-3f and whose conic is robustly positive definite stays below
alpha = 1e-3f on every pixel of its AABB (float32 numpy, test_gpu_parity.max_alpha_on_tiles).
That is what lets the GPU tests demand the oracle's image, take maps and lists of a frame
with those Gaussians removed.

One honest limit.  In searches of up to 4,096 needle-thin Gaussians, with scales down to 5e-5
and 1e-7, no low-opacity Gaussian that FAILS the robust-PD test reached alpha >= 1e-3 on a
pixel.  So no image can show that the PD clause of the cull is necessary; the record-level
checks of test_gpu_temporal.py pin it instead (such a Gaussian must keep its record)."""
import numpy as np
import pytest

import _temporal_scenes as ts
from test_gpu_parity import CAMS, cam_for, max_alpha_on_tiles

W, H = ts.W, ts.H
TINY = np.finfo(np.float32).tiny

# (scene, camera, time) of every case of test_gpu_temporal.py's record test
RECORD_CASES = ([("t_slabs", ci, t) for t in ts.TIMES for ci in (0, 2)]
                + [("t_needles_band", ci, ts.T0) for ci in (0, 2)]
                + [("t_slabs_band", ci, ts.T0) for ci in range(4)]
                + [("edges", ci, ts.T0) for ci in (0, 2)] + [("boundary", 0, ts.T0)])

_cache = {}


def case(gsr, orc, name, ci, t):
    """The oracle's view of one case, once per process and left unchanged: the 3D scene at t,
    the camera, the records and what they say about the temporal cull."""
    key = (name, ci, t)
    if key not in _cache:
        soa3 = orc.temporal(ts.scene(name), t)
        cam = cam_for(gsr, W, H, **CAMS[ci])
        want = orc.preprocess(soa3, cam, W, H, 3.0)
        for a in (soa3, want):
            a.setflags(write=False)
        op = want["opacity"]
        with np.errstate(invalid="ignore"):
            between = (want["status"] == 2) & (op >= ts.CULL_OPACITY) & (op < ts.TAKE_ALPHA)
        _cache[key] = dict(soa3=soa3, cam=cam, want=want, vis=want["status"] == 2, low=ts.low_opacity(want),
                           pd=ts.robust_pd(want), between=between, culled=ts.cull_predicate(want))
    return _cache[key]


def tiny_opacities(soa3):
    """Temporal opacities that are subnormal or zero."""
    return int((np.abs(soa3[ts.A_OPACITY]) < TINY).sum())


@pytest.mark.parametrize("ci", [0, 2])
def test_needles_band_straddles_threshold_and_pd_test(gsr, orc, ci):
    c = case(gsr, orc, "t_needles_band", ci, ts.T0)
    low_pd, low_npd, between = int((c["low"] & c["pd"]).sum()), int((c["low"] & ~c["pd"]).sum()), int(c["between"].sum())
    print(f"t_needles_band camera {ci}: low & pd {low_pd} (floor 500), low & ~pd {low_npd} (floor 50), "
          f"opacity in [0.9e-3, 1e-3) {between} (floor 30)")
    assert low_pd >= 500 and low_npd >= 50 and between >= 30


@pytest.mark.parametrize("ci", range(len(CAMS)))
def test_slabs_band_straddles_threshold(gsr, orc, ci):
    c = case(gsr, orc, "t_slabs_band", ci, ts.T0)
    low, between = int(c["low"].sum()), int(c["between"].sum())
    print(f"t_slabs_band camera {ci}: low {low} (floor 90), opacity in [0.9e-3, 1e-3) {between} (floor 8)")
    assert low >= 90 and between >= 8


@pytest.mark.parametrize("t", ts.TIMES)
def test_slabs_over_time(gsr, orc, t):
    """Times inside and outside [0, 1]: at least 100 low-opacity Gaussians each, and temporal
    factors that underflow to subnormal and zero opacities."""
    floor_tiny = {0.0: 20, -0.5: 100, 1.6: 100}.get(t, 0)
    for ci in (0, 2):
        c = case(gsr, orc, "t_slabs", ci, t)
        low, tiny = int(c["low"].sum()), tiny_opacities(c["soa3"])
        print(f"t_slabs t {t:g} camera {ci}: low {low} (floor 100), subnormal or zero opacities {tiny} "
              f"(floor {floor_tiny})")
        assert low >= 100 and tiny >= floor_tiny


def test_the_pd_test_is_the_same_in_float32(gsr, orc):
    """The float64 classification and the kernel's float32 statement of it agree on every
    visible record of every case: no case sits on the PD test's own rounding."""
    for name, ci, t in RECORD_CASES:
        c = case(gsr, orc, name, ci, t)
        assert np.array_equal(ts.robust_pd(c["want"], np.float32)[c["vis"]], c["pd"][c["vis"]]), (name, ci, t)


def test_boundary(gsr, orc):
    soa = ts.scene("boundary")
    c = case(gsr, orc, "boundary", 0, ts.T0)
    ops = ts.boundary_opacities()
    assert (np.diff(ops.view(np.uint32).astype(np.int64)) > 0).all() and ops[1] == ts.CULL_OPACITY and ops[4] == ts.TAKE_ALPHA
    # orc.temporal returns the stored opacities bit for bit, whatever trbf_scale
    assert np.array_equal(c["soa3"][ts.A_OPACITY].view(np.uint32), soa[ts.A_OPACITY].view(np.uint32))
    assert np.array_equal(np.unique(soa[ts.A_TSCALE]), np.array([1e-30, 0.05, 1.0, 1e30], np.float32))
    want = c["want"]
    assert c["vis"].all()
    assert np.array_equal(want["opacity"].view(np.uint32), soa[ts.A_OPACITY].view(np.uint32))
    assert np.array_equal(np.nonzero(c["culled"])[0], np.arange(8))         # only those below 0.9e-3f
    _, takes = orc.render_takes(c["soa3"], c["cam"], W, H, 3.0)
    count = (takes & np.uint64(0xFFFFFFFF)).astype(np.int64)
    at_centre = count[want["px_y"], want["px_x"]].reshape(6, 8).sum(axis=1)
    print("boundary: takes at the centres per opacity value", at_centre.tolist(), "pixels with a take", int((count > 0).sum()))
    assert at_centre.tolist() == [0, 0, 0, 0, 8, 8]
    assert (count > 0).sum() == 16 and count.max() == 1
    assert (count[want["px_y"][32:], want["px_x"][32:]] == 1).all()


def test_edges(gsr, orc):
    soa3 = orc.temporal(ts.scene("edges"), ts.T0)
    g = ts.edge_group(soa3.shape[1])
    op, pos = soa3[ts.A_OPACITY], soa3[0:3]
    stored = ts.scene("edges")[ts.A_OPACITY]
    for k in (0, 4):          # temporal factor exactly 1
        assert np.array_equal(op[g == k].view(np.uint32), stored[g == k].view(np.uint32)), k
    assert (op[g == 1] == 0).all() and (op[g == 2] == 0).all()
    assert np.isnan(op[g == 3]).all()
    o5 = op[g == 5]
    sub, zero = int(((o5 != 0) & (np.abs(o5) < TINY)).sum()), int((o5 == 0).sum())
    inf6, nan6 = int(np.isinf(pos[:, g == 6]).sum()), int(np.isnan(pos[:, g == 6]).sum())
    print(f"edges: group 5 subnormal {sub} (floor 10), zero {zero} (floor 5); group 6 position components "
          f"+-inf {inf6}, NaN {nan6} (floor 1 each)")
    assert sub >= 10 and zero >= 5 and inf6 >= 1 and nan6 >= 1
    assert np.isfinite(pos[:, g != 6]).all()
    for ci in (0, 2):
        c = case(gsr, orc, "edges", ci, ts.T0)
        assert not c["vis"][g == 6].any()
        lost7 = int((c["want"]["status"][g == 7] == 0).sum())
        print(f"edges camera {ci}: group 7 without a record {lost7} (floor 4), visible {int(c['vis'].sum())}, "
              f"visible with NaN opacity {int(c['vis'][g == 3].sum())}")
        assert lost7 >= 4 and c["vis"][g == 3].sum() >= 16
        assert np.isfinite(orc.render(c["soa3"], c["cam"], W, H, 3.0)).all()
    nan_only = orc.temporal(ts.scene("edges_nan"), ts.T0)
    assert nan_only.shape[1] == 32 and np.isnan(nan_only[ts.A_OPACITY]).all()


@pytest.mark.parametrize("name,ci,t", RECORD_CASES)
def test_low_opacity_pd_gaussians_stay_below_the_alpha_threshold(gsr, orc, name, ci, t):
    """The temporal cull's proof on the reference side: the largest alpha of every low & pd
    Gaussian over every pixel of its AABB stays below 1e-3f."""
    c = case(gsr, orc, name, ci, t)
    who = c["low"] & c["pd"]
    pairs = ts.subset_pairs(orc, c["want"], who)
    peak = max_alpha_on_tiles(c["want"], pairs, W)
    print(f"{name} camera {ci} t {t:g}: low & pd {int(who.sum())} of {int(c['vis'].sum())} visible, {pairs.size} pairs, "
          f"largest alpha {float(peak.max(initial=0.0)):.4e}")
    assert who.sum() >= 8 and pairs.size >= who.sum()
    assert (peak < ts.TAKE_ALPHA).all()
