"""The numpy twins of the scene initialisation (tests/_points_ref.py) pinned on the CPU: the
float32 k-NN statistic against a float64 brute force of the same inputs, its edge rules on
hand-made clouds, and the fill against a restatement of 3DGS's create_from_pcd pushed through the
loader's activations."""
import numpy as np
import pytest

import _points_ref as ref

U = 2.0 ** -24   # the unit roundoff of float32


@pytest.mark.parametrize("n,seed", [(4097, 1), (3000, 2)])
def test_knn_twin_against_float64(n, seed):
    """Relative difference <= 9 * 2^-24.  Eight roundings lie on the path: one in the
    difference, one in the square, two in the sum of squares, two in the sum of three, one in
    the division, and one for the float32 choice among near-ties (a different neighbour can be
    chosen only when its distance is within the same terms).  The ninth unit covers the
    second-order terms.  Clouds without coincident points or denormal distances."""
    rng = np.random.default_rng(seed)
    xyz = ref.clustered(rng, n) if seed == 1 else rng.uniform(-3, 3, (n, 3)).astype(np.float32)
    got, bad = ref.knn_dist2(xyz)
    want = ref.knn_dist2_f64(xyz)
    assert bad == 0 and got.dtype == np.float32
    assert want.min() > 1e-30, "coincident points or denormal distances in the cloud"
    rel = np.abs(got.astype(np.float64) - want) / want
    print(f"n = {n}: max relative difference {rel.max() / U:.2f} * 2^-24")
    assert rel.max() <= 9 * U
    if seed == 1:
        assert want.max() / want.min() > 1e6     # the densities do span decades


def test_knn_twin_chunking_and_rows():
    rng = np.random.default_rng(3)
    xyz = ref.clouds(rng, 700)["nonfinite"]
    a, bad = ref.knn_dist2(xyz, chunk=1024)
    b, _ = ref.knn_dist2(xyz, chunk=37)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and bad >= 3
    rows = rng.choice(700, 50, replace=False)
    assert np.array_equal(ref.knn_rows(xyz, rows).view(np.uint32), a[rows].view(np.uint32))


def test_knn_twin_rules():
    f = np.float32
    # k = 0, 1, 2: nothing, the one distance, the mean of two
    assert ref.knn_dist2(np.zeros((0, 3), f))[0].size == 0
    assert ref.knn_dist2(f([[1, 2, 3]]))[0].tolist() == [0.0]
    assert ref.knn_dist2(f([[0, 0, 0], [3, 4, 0]]))[0].tolist() == [25.0, 25.0]
    got = ref.knn_dist2(f([[0, 0, 0], [1, 0, 0], [0, 2, 0]]))[0]
    assert got.tolist() == [f(2.5), f(3.0), f(4.5)]
    # k = 3 as a multiset: coincident points are neighbours at distance 0
    got = ref.knn_dist2(f([[0, 0, 0]] * 3 + [[1, 0, 0], [5, 0, 0]]))[0]
    assert got[:3].tolist() == [f(1.0) / f(3.0)] * 3 and got[3] == f(1.0)
    # invalid points: nobody's neighbour, +0 themselves, counted; k follows the valid count
    xyz = f([[0, 0, 0], [np.nan, 0, 0], [1, 0, 0], [0, np.inf, 0], [0, 3, 0], [0, 0, -np.inf]])
    got, bad = ref.knn_dist2(xyz)
    assert bad == 3 and got.tolist() == [5.0, 0.0, 5.5, 0.0, 9.5, 0.0]
    assert not np.signbit(got).any()
    # overflow propagates
    big = f([[3e19, 0, 0], [-3e19, 0, 0], [0, 3e19, 0], [0, -3e19, 0]])
    assert np.isinf(ref.knn_dist2(big)[0]).all()
    # every cloud of the GPU tests has the shape and the planted values it claims
    for n in (5, 1000):
        cl = ref.clouds(np.random.default_rng(n), n)
        assert len(cl) == 12 and all(v.shape == (n, 3) and v.dtype == f for v in cl.values())
        assert (~ref.valid_mask(cl["nonfinite"])).sum() == max(3, n // 100)
        assert all(ref.valid_mask(v).all() for k, v in cl.items() if k != "nonfinite")


def test_fill_twin_against_create_from_pcd():
    """3DGS's create_from_pcd stores raw values (float32) that the loader activates:
      f_dc     = RGB2SH(rgb) = (rgb - 0.5) / C0
      scale    = log(sqrt(clamp_min(dist2, 1e-7)))     -> exp
      opacity  = inverse_sigmoid(0.1) = log(0.1 / 0.9) -> 1 / (1 + exp(-v))
      rotation = (1, 0, 0, 0)
    The twin stores the activated values directly.  Bounds, in units of u = 2^-24, relative:
      scale:   the twin rounds once (the correctly rounded root; max and the factor 1 are exact);
               the restatement rounds the raw value r to float32, |dr| <= |r| u, and exp turns
               an absolute error of the argument into a relative one of the value: (1 + |r|) u,
               asserted as (2 + |r|) u for the second-order terms.
      opacity: float32(0.1) is within u; the raw value's rounding, |r| u with |r| = 2.197, is
               scaled by d log(sigmoid) / dr = 1 - 0.1 = 0.9: 1.98 u.  Asserted as 4 u.
      dc:      the twin rounds the difference, the constant C0 and the quotient (3 u); the
               restatement rounds the stored raw value (u).  Asserted as 5 u."""
    rng = np.random.default_rng(5)
    n = 2000
    xyz = ref.clustered(rng, n)
    rgb = rng.uniform(0, 1, (n, 3)).astype(np.float32)
    rgb[:3] = [[0.5, 0.0, 1.0], [0.25, 0.75, 0.5], [1e-3, 0.999, 0.5]]
    mean2, _ = ref.knn_dist2(xyz)
    mean2[:2] = [0.0, 1e-9]                               # below the floor
    for narrays in (38, 49, 59):
        soa = ref.fill(xyz, rgb, mean2, narrays, t_center=0.25, t_scale=0.5)
        assert soa.shape == (narrays, n) and soa.dtype == np.float32
        assert np.array_equal(soa[0:3].view(np.uint32), xyz.T.view(np.uint32))
        raw_scale = np.log(np.sqrt(np.maximum(mean2.astype(np.float64), 1e-7))).astype(np.float32).astype(np.float64)
        want_scale = np.exp(raw_scale)
        for c in range(3):
            rel = np.abs(soa[4 + c].astype(np.float64) - want_scale) / want_scale
            assert (rel <= (2 + np.abs(raw_scale)) * U).all()
        assert soa[4, 0] == soa[4, 1] == np.sqrt(np.float32(1e-7))
        raw_op = float(np.float32(np.log(0.1 / 0.9)))
        want_op = 1.0 / (1.0 + np.exp(-raw_op))
        assert (soa[3] == np.float32(0.1)).all() and abs(float(soa[3, 0]) - want_op) / want_op <= 4 * U
        assert (soa[7] == 1.0).all() and not soa[8:11].view(np.uint32).any()
        want_dc = ((rgb.astype(np.float64) - 0.5) / 0.28209479177387814).astype(np.float32).astype(np.float64)
        assert (np.abs(soa[11:14].T.astype(np.float64) - want_dc) <= 5 * U * np.abs(want_dc)).all()
        assert soa[11, 0] == 0.0 and soa[13, 1] == 0.0    # rgb 0.5: exactly +0
        rest_end = 38 if narrays != 59 else 59
        assert not soa[14:rest_end].view(np.uint32).any()
        if narrays == 49:
            assert (soa[38] == 0.25).all() and (soa[39] == 0.5).all() and not soa[40:49].view(np.uint32).any()
    # no colours: grey, dc exactly +0; the cap and the factor
    soa = ref.fill(xyz, None, mean2, 38, scale_mul=2.0, scale_max=0.01)
    assert not soa[11:14].view(np.uint32).any()
    s = np.sqrt(np.maximum(mean2, np.float32(1e-7))) * np.float32(2.0)
    assert np.array_equal(soa[4], np.minimum(s, np.float32(0.01))) and (soa[4] == np.float32(0.01)).any()
    assert (soa[4] < np.float32(0.01)).any()
