"""The densification sampler (include/gsr_detmath.h: gsr_logf, gsr_philox4x32_10, the Box-Muller
normals behind gsr_densify_normals) and the numpy twin of the densify call (tests/_densify_ref.py)
on a CPU-only host: known answers, accuracy against float64, the sample's statistics, and the
twin against a restatement of 3DGS's densify_and_clone / densify_and_split / prune."""
import math

import numpy as np
import pytest

import _densify_ref as ref
from test_detmath import ulp_err, vec

R_MAX = math.sqrt(48.0 * math.log(2.0))   # sqrt(-2 ln 2^-24): the largest radius the sampler draws


# ---------------------------------------------------------------- Philox

KAT = [
    ([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0],
     [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
]


@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox_known_answers(counter, key, want):
    got = ref.philox4x32_10([np.uint32(c) for c in counter], [np.uint32(k) for k in key])
    assert [int(x) for x in got] == want
    # and as one lane of a vector call
    cs = [np.array([1, c, 7], np.uint32) for c in counter]
    assert [int(x) for x in ref.philox4x32_10(cs, [np.uint32(k) for k in key])[:, 1]] == want


# ---------------------------------------------------------------- gsr_logf

def test_logf_within_2_ulp_over_every_sampler_input(gsr):
    """u = k 2^-24 for k = 1 .. 2^24 is every value the sampler hands to gsr_logf: at most 2 ulp
    against float64, the bound tests/test_detmath.py holds gsr_expf to."""
    L = gsr.lib()
    worst = 0.0
    step = 1 << 20
    for k0 in range(0, 1 << 24, step):
        u = (np.arange(k0 + 1, k0 + step + 1, dtype=np.float64) * 2.0 ** -24).astype(np.float32)
        out = np.empty_like(u)
        assert L.gsr_logf_probe(u.ctypes.data, u.size, out.ctypes.data) == 0
        worst = max(worst, float(ulp_err(out, np.log(u.astype(np.float64))).max()))
    print(f"gsr_logf: max {worst:.4f} ulp over the 2^24 sampler inputs")
    assert worst <= 2.0
    assert L.gsr_logf_probe(None, 4, None) == -1 and L.gsr_logf_probe(u.ctypes.data, -1, out.ctypes.data) == -1


# ---------------------------------------------------------------- the normals

def test_normals_agree_with_float64_box_muller(gsr, orc):
    """gsr_densify_normals against float64 Box-Muller (exact u, v and 2 pi) on the numpy Philox.

    Tolerance, from the parts' own bounds (R = sqrt(48 ln 2) = 5.768 bounds every radius):
      radius  L = gsr_logf(u) is within 2 ulp, a relative 2 * 2^-23; -2 L is exact; the square
              root halves the relative error and sqrtf rounds once more: r is within
              rho = 2^-23 + 2^-24 of sqrt(-2 ln u), an absolute R * rho = 1.03e-6.
      angle   a = fl(6.2831855f * v): the constant is float32(2 pi) = 2 pi + 1.75e-7, v < 1 is
              exact and the product below 8 rounds by at most 2^-22 = 2.38e-7: |a - 2 pi v| <=
              4.14e-7, which moves cos and sin by no more than that.
      trig    tests/test_detmath.py asserts |gsr_sinf - sin|, |gsr_cosf - cos| <= max(2 ulp, 1e-9)
              on [-pi, pi]; the angles here reach 2 pi, so this test first checks that same
              bound on [0, 2 pi).  With results in [-1, 1] it is at most 2 * 2^-23 = 2.38e-7.
      product z = fl(r * trig) rounds once more: R * 2^-24 = 3.4e-7.
    Sum: R * (4.14e-7 + 2.38e-7) + 1.03e-6 + 3.4e-7 = 5.1e-6, plus 0.1 % for the products of
    two error terms.  (The issue's estimate was "below 1e-5".)"""
    L = orc.lib()
    a = np.linspace(0.0, 2.0 * math.pi, 100_001, dtype=np.float32)[:-1]
    for f, r in ((L.orc_sinf, np.sin), (L.orc_cosf, np.cos)):
        want = r(a.astype(np.float64))
        err = np.abs(vec(f, a).astype(np.float64) - want)
        assert (err <= np.maximum(2.0 * np.spacing(np.abs(want.astype(np.float32))).astype(np.float64), 1e-9)).all()

    two_pi32 = float(np.float32(2.0 * math.pi))
    angle = (two_pi32 - 2.0 * math.pi) + 2.0 ** -22
    tol = (R_MAX * (angle + 2.0 * 2.0 ** -23) + R_MAX * (2.0 ** -23 + 2.0 ** -24) + R_MAX * 2.0 ** -24) * 1.001
    assert 5.0e-6 < tol < 5.2e-6
    worst = 0.0
    for seed in (0, 1, 0xDEADBEEF12345678, 2 ** 64 - 1):
        idx = np.concatenate([np.arange(1000), [2 ** 31 - 1, 2 ** 32 - 1]]).astype(np.uint32).repeat(2)
        child = np.tile(np.array([0, 1], np.uint32), idx.size // 2)
        got = gsr.densify_normals(seed, idx, child)
        want = ref.box_muller64(ref.child_words(seed, idx, child))
        assert got.dtype == np.float32 and got.shape == want.shape
        worst = max(worst, float(np.abs(got.astype(np.float64) - want).max()))
    print(f"densify normals: max |z - float64 Box-Muller| = {worst:.3g} (tolerance {tol:.3g})")
    assert worst <= tol


@pytest.fixture(scope="module")
def sample(gsr):
    """2^20 children: both children of the sources 0 .. 2^19 - 1 under one seed."""
    idx = np.arange(1 << 19, dtype=np.uint32).repeat(2)
    child = np.tile(np.array([0, 1], np.uint32), 1 << 19)
    return gsr.densify_normals(20240229, idx, child)


def test_sample_statistics(sample):
    N = sample.shape[0]
    assert N == 1 << 20
    z = sample.astype(np.float64)
    for c in range(3):
        mean, var = z[:, c].mean(), z[:, c].var()
        print(f"component {c}: mean {mean:+.5f} var {var:.5f} max |z| {np.abs(z[:, c]).max():.4f}")
        assert abs(mean) <= 5.0 / math.sqrt(N)
        assert abs(var - 1.0) <= 5.0 * math.sqrt(2.0 / N)
        assert np.abs(z[:, c]).max() <= R_MAX * (1.0 + 1e-6)


def test_children_and_seeds_differ(gsr, sample):
    assert (sample[0::2] != sample[1::2]).any(axis=1).all()          # children (i, 0) and (i, 1)
    idx = np.arange(4096, dtype=np.uint32)
    other = gsr.densify_normals(20240230, idx, np.zeros(4096, np.uint32))
    assert (other != sample[0:8192:2]).any(axis=1).all()
    again = gsr.densify_normals(20240229, idx, np.zeros(4096, np.uint32))
    assert np.array_equal(again.view(np.uint32), sample[0:8192:2].view(np.uint32))
    # the high word of the seed is part of the key
    hi = gsr.densify_normals(20240229 + (1 << 32), idx, np.zeros(4096, np.uint32))
    assert (hi != again).any(axis=1).all()
    one = gsr.densify_normals(20240229, 5, 1)
    assert one.shape == (3,) and np.array_equal(one, sample[11])


# ---------------------------------------------------------------- the twin against 3DGS

def random_case(rng, narrays, n):
    soa = rng.normal(0, 1, (narrays, n))
    soa[3] = rng.uniform(0.0, 1.0, n)                          # opacity: some below min_opacity
    soa[4:7] = np.exp(rng.uniform(-5.0, -1.0, (3, n)))         # scales around the split threshold
    soa[7:11] = rng.normal(0, 1, (4, n))
    if narrays == 49:
        soa[39] = np.exp(rng.uniform(-3, 0, n))
    seen = rng.integers(0, 4, n).astype(np.uint32)
    accum = (rng.exponential(0.0004, n) * np.maximum(seen, 1)).astype(np.float32)
    return soa, accum, seen


def gs3d_reference(soa, grads, cfg, z0, z1):
    """3DGS's densify_and_clone, densify_and_split (N = 2) and prune restated in torch float64 on
    (n, narrays) rows; z0 / z1: the standard normals of every source's two children, which stand
    in for torch.normal(0, stds) = z * stds."""
    import torch
    P = torch.from_numpy(np.ascontiguousarray(soa.T))
    n = P.shape[0]
    grads = torch.from_numpy(grads)
    z = [torch.from_numpy(z0), torch.from_numpy(z1)]
    scaling = lambda Q: Q[:, 4:7]

    # densify_and_clone
    sel = (grads >= cfg["grad_threshold"]) & (scaling(P).max(dim=1).values <= cfg["scale_split"])
    P1 = torch.cat([P, P[sel]])

    # densify_and_split: the gradients are padded with zeros for the clones
    padded = torch.zeros(P1.shape[0], dtype=torch.float64)
    padded[:n] = grads
    sel = (padded >= cfg["grad_threshold"]) & (scaling(P1).max(dim=1).values > cfg["scale_split"])
    par = P1[sel]
    stds = scaling(par).repeat(2, 1)
    zsel = torch.cat([z[0][sel[:n].nonzero()[:, 0]], z[1][sel[:n].nonzero()[:, 0]]])
    samples = zsel * stds
    q = par[:, 7:11]
    q = q / q.norm(dim=1, keepdim=True)
    r, x, y, k = q[:, 0], q[:, 1], q[:, 2], q[:, 3]                       # build_rotation (k: the z part)
    R = torch.stack([1 - 2 * (y * y + k * k), 2 * (x * y - r * k), 2 * (x * k + r * y),
                     2 * (x * y + r * k), 1 - 2 * (x * x + k * k), 2 * (y * k - r * x),
                     2 * (x * k - r * y), 2 * (y * k + r * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)
    new = par.repeat(2, 1)
    new[:, 0:3] = torch.bmm(R.repeat(2, 1, 1), samples.unsqueeze(-1)).squeeze(-1) + par[:, 0:3].repeat(2, 1)
    new[:, 4:7] = scaling(par).repeat(2, 1) / (0.8 * 2)
    assert cfg["split_shrink"] == 1.6
    P2 = torch.cat([P1[~sel], new])

    # prune
    drop = (P2[:, 3] < cfg["min_opacity"]) | (scaling(P2).max(dim=1).values > cfg["prune_scale_max"])
    return P2[~drop].numpy()


def sorted_rows(a):
    return a[np.lexsort(a.T[::-1])]


@pytest.mark.parametrize("narrays", [38, 49])
def test_twin_matches_3dgs(gsr, narrays):
    rng = np.random.default_rng(narrays)
    n = 3000
    soa, accum, seen = random_case(rng, narrays, n)
    cfg = dict(ref.CFG_3DGS, prune_scale_max=0.3, seed=99)
    normals = lambda i, k: gsr.densify_normals(cfg["seed"], i, k)
    block, src, kind, rep = ref.densify(soa, accum, seen, cfg, normals, dtype=np.float64)
    assert min(rep["kept"], rep["cloned"], rep["split"], rep["pruned"]) > 50, rep
    assert rep["n_out"] == block.shape[1] == rep["kept"] + 2 * (rep["cloned"] + rep["split"])
    assert rep["kept"] + rep["cloned"] + rep["split"] + rep["pruned"] == n

    grads = np.where(seen != 0, accum.astype(np.float64) / np.maximum(seen, 1), 0.0)
    allsrc = np.arange(n)
    z0 = normals(allsrc, np.zeros(n)).astype(np.float64)
    z1 = normals(allsrc, np.ones(n)).astype(np.float64)
    want = gs3d_reference(soa, grads, cfg, z0, z1)
    got = block.T
    assert got.shape == want.shape
    # as multisets: 3DGS appends the clones and the children at the end
    np.testing.assert_allclose(sorted_rows(got), sorted_rows(want), rtol=1e-12, atol=1e-12)


def test_twin_order_and_kinds(gsr):
    """The expansion order of the twin itself: sources ascending, one source's outputs adjacent,
    kinds 0 | 0, 1 | 2, 3; float32 children differ from their parent in six planes only."""
    rng = np.random.default_rng(5)
    soa, accum, seen = random_case(rng, 38, 500)
    soa = soa.astype(np.float32)
    cfg = dict(ref.CFG_3DGS, seed=3)
    block, src, kind, rep = ref.densify(soa, accum, seen, cfg, lambda i, k: gsr.densify_normals(3, i, k))
    assert block.dtype == np.float32 and (np.diff(src) >= 0).all()
    for i in range(500):
        ks = kind[src == i].tolist()
        assert ks in ([], [0], [0, 1], [2, 3])
    same = block.view(np.uint32) == soa[:, src].view(np.uint32)
    assert same[:, kind < 2].all()
    kids = kind >= 2
    assert same[[3] + list(range(7, 38))][:, kids].all() and not same[4:7][:, kids].any()
