"""Hand-made spacetime scenes — TEST INFRASTRUCTURE.

gsr_synth_write_ply4d's Gaussians are well-conditioned few-pixel splats with trbf_scale in
exp(U(-3.5, -2)), small motion and times in [0, 1], so they reach neither the boundary of the
4D preprocess's temporal cull (opacity at t next to 0.9e-3 and 1e-3, conics on both sides of
the robust-PD test) nor the edge values of its temporal arithmetic (dt = 0, a trbf_scale of
0, 1e-30 or 1e30, a temporal factor that goes subnormal and then 0, motion through the near
plane or to +-inf / NaN).  The scenes below give the splats of tests/_wide_scenes.py a time
axis that does (tests/test_temporal_scenes.py asserts it on the oracle's records alone).

Every builder returns a (49, n) float32 array for Scene.from_soa and orc.temporal alike: the
38 arrays of the 3D scene, then trbf_center, trbf_scale and motion_0..8.  One generator per
builder, drawn in the documented order."""
from __future__ import annotations

import numpy as np

import _wide_scenes as ws

W, H = ws.W, ws.H
A_OPACITY, A_TCENTER, A_TSCALE, A_MOTION0 = 3, 38, 39, 40
F = np.float32

CULL_OPACITY = F(0.9e-3)      # the temporal cull's threshold (gsr_kernels.hip preprocess_camera)
TAKE_ALPHA = F(1e-3)          # the blend's (render.cu:335)
TIMES = (0.0, 0.3, 0.7, -0.5, 1.6)
T0 = 0.4


def _with_time_axis(soa38):
    soa = np.zeros((49, soa38.shape[1]), np.float32)
    soa[:38] = soa38
    return soa


def to4d(soa38, seed):
    """Any 3D scene with a time axis: trbf_center U(0, 1), trbf_scale log-uniform(0.02, 0.5),
    motion_0..2 ~ N(0, 0.3), motion_3..5 ~ N(0, 0.1), motion_6..8 ~ N(0, 0.05), drawn in
    that order."""
    rng = np.random.default_rng(seed)
    soa = _with_time_axis(soa38)
    n = soa.shape[1]
    soa[A_TCENTER] = rng.uniform(0.0, 1.0, n)
    soa[A_TSCALE] = np.exp(rng.uniform(np.log(0.02), np.log(0.5), n))
    for j, sd in enumerate((0.3, 0.1, 0.05)):
        soa[A_MOTION0 + 3 * j:A_MOTION0 + 3 * j + 3] = rng.normal(0.0, sd, (3, n))
    return soa


def band(soa38, t0, seed):
    """No motion, trbf_scale 0.1, and trbf_center chosen per Gaussian so that its temporal
    opacity at t0 is log-uniform in [2e-4, 5e-3], a band around the cull's 0.9e-3 and the
    blend's 1e-3: with u = sqrt(-ln(target / op)), center = t0 - 0.1 u.  A Gaussian whose
    stored opacity is already below its target gets dt = 0."""
    rng = np.random.default_rng(seed)
    soa = _with_time_axis(soa38)
    n = soa.shape[1]
    target = np.exp(rng.uniform(np.log(2e-4), np.log(5e-3), n))
    op = soa[A_OPACITY].astype(np.float64)
    with np.errstate(all="ignore"):
        u = np.sqrt(-np.log(target / op))
    soa[A_TSCALE] = 0.1
    soa[A_TCENTER] = np.where(op > target, t0 - 0.1 * u, t0)
    return soa


def boundary_opacities():
    """The six stored opacities of boundary(): the float32 neighbour below 0.9e-3f, 0.9e-3f,
    its neighbour above, the neighbour below 1e-3f, 1e-3f, its neighbour above."""
    lo, hi = F(-np.inf), F(np.inf)
    return np.array([np.nextafter(CULL_OPACITY, lo), CULL_OPACITY, np.nextafter(CULL_OPACITY, hi),
                     np.nextafter(TAKE_ALPHA, lo), TAKE_ALPHA, np.nextafter(TAKE_ALPHA, hi)], np.float32)


def boundary(t0):
    """48 isotropic Gaussians (scale 0.05, identity quaternion, f_dc 1) on an 8 x 6 grid over
    x in [-1.6, 1.6], y in [-1, 1] at z = 0.  trbf_center = t0 exactly, so dt = 0, the
    temporal factor is 1 and the temporal opacity is the stored opacity bit for bit, whatever
    trbf_scale (which cycles through 1e-30, 0.05, 1, 1e30).  Grid row r (Gaussians 8 r ..
    8 r + 7) carries boundary_opacities()[r]."""
    soa = np.zeros((49, 48), np.float32)
    gx, gy = np.meshgrid(np.linspace(-1.6, 1.6, 8), np.linspace(-1.0, 1.0, 6))
    soa[0], soa[1] = gx.ravel(), gy.ravel()
    soa[A_OPACITY] = np.repeat(boundary_opacities(), 8)
    soa[4:7] = 0.05
    soa[7] = 1.0
    soa[11:14] = 1.0
    soa[A_TCENTER] = t0
    soa[A_TSCALE] = np.tile(np.array([1e-30, 0.05, 1.0, 1e30], np.float32), 12)
    return soa


EDGE_GROUPS = 8


def edge_group(n):
    return np.arange(n) % EDGE_GROUPS


def edges(t0, seed):
    """to4d(slabs) with Gaussian i in group i % 8:
      0  dt = 0 with trbf_scale 1e-30            (0 / 1e-30 = 0: temporal factor 1)
      1  trbf_scale 1e-30, dt != 0               (u * u = inf: temporal opacity 0)
      2  trbf_scale 0, dt != 0                   (u = +-inf: temporal opacity 0)
      3  trbf_scale 0, dt = 0                    (0 / 0: NaN opacity)
      4  trbf_scale 1e30                         (u * u underflows to 0: temporal factor 1)
      5  u * u uniform in [80, 110]              (the temporal factor goes subnormal, then 0)
      6  motions of +-3.4e38, |dt| 0.9 or 1.1    (0.9: the products stay finite and their sums
                                                 overflow to +-inf; 1.1: the products are
                                                 +-inf themselves, opposite signs give NaN)
      7  motion_2 uniform in +-40                (through the near plane and behind the camera)"""
    soa = to4d(ws.scene("slabs"), seed)
    rng = np.random.default_rng(seed + 1)
    n = soa.shape[1]
    g = edge_group(n)
    t0 = F(t0)
    # to4d's centres are U(0, 1): move one that happens to equal t0, so that dt != 0 holds
    soa[A_TCENTER, soa[A_TCENTER] == t0] += F(0.25)
    soa[A_TCENTER, (g == 0) | (g == 3)] = t0
    soa[A_TSCALE, (g == 0) | (g == 1)] = 1e-30
    soa[A_TSCALE, (g == 2) | (g == 3)] = 0.0
    soa[A_TSCALE, g == 4] = 1e30
    m = g == 5
    soa[A_TCENTER, m] = t0 - soa[A_TSCALE, m].astype(np.float64) * np.sqrt(rng.uniform(80.0, 110.0, int(m.sum())))
    m = g == 6
    soa[A_TCENTER, m] = t0 + rng.choice(np.array([-1.1, -0.9, 0.9, 1.1], np.float32), int(m.sum()))
    soa[A_MOTION0:A_MOTION0 + 9, m] = F(3.4e38) * rng.choice(np.array([-1.0, 1.0], np.float32), (9, int(m.sum())))
    m = g == 7
    soa[A_MOTION0 + 2, m] = rng.uniform(-40.0, 40.0, int(m.sum()))
    return soa


# name: builder.  Seeds are fixed here; what a case reaches is asserted per case in
# tests/test_temporal_scenes.py.
_BUILDERS = {
    "t_slabs": lambda: to4d(ws.scene("slabs"), 105),
    "t_stack": lambda: to4d(ws.scene("stack"), 109),
    "t_needles_band": lambda: band(ws.scene("needles", n=2048, scales=(1e-4, 2.0)), T0, 206),
    "t_slabs_band": lambda: band(ws.scene("slabs"), T0, 202),
    "boundary": lambda: boundary(T0),
    "edges": lambda: edges(T0, 305),
    "edges_nan": lambda: np.ascontiguousarray(edges(T0, 305)[:, edge_group(256) == 3]),
}
_scenes = {}


def scene(name):
    """A scene of this module by name, built once and read-only."""
    if name not in _scenes:
        _scenes[name] = _BUILDERS[name]()
        _scenes[name].setflags(write=False)
    return _scenes[name]


# ---------------------------------------------------------------- what the oracle's records say

def low_opacity(want):
    """Visible with opacity < 0.9e-3f (NaN: not low)."""
    with np.errstate(invalid="ignore"):
        return (want["status"] == 2) & (want["opacity"] < CULL_OPACITY)


def robust_pd(want, dtype=np.float64):
    """a > 0, e > 0, a e - h^2 > 1e-4 a e with h = (b + c) / 2 on the records' conics.  With
    dtype float32 every operation rounds once, as in the kernels' translation units (built
    with -ffp-contract=off): the temporal cull's own statement of it."""
    a, b, c, e = (want["inv_covar"][:, j].astype(dtype) for j in range(4))
    with np.errstate(all="ignore"):
        h = dtype(0.5) * (b + c)
        return (a > 0) & (e > 0) & ((a * e - h * h) > dtype(1e-4) * (a * e))


def cull_predicate(want):
    """The documented temporal cull on the oracle's records, in float32:
    opt < 0.9e-3f && a > 0 && e > 0 && (a*e - h*h) > 1e-4f * (a*e), h = 0.5f * (b + c)."""
    return low_opacity(want) & robust_pd(want, np.float32)


def subset_pairs(orc, want, mask, Wf=W, Hf=H):
    """ws.rect_pairs of the visible Gaussians in mask alone."""
    w = want.copy()
    w["status"][~mask] = 0
    return ws.rect_pairs(w, orc.expected_depth_order(w), Wf, Hf)


def without(want, culled):
    """The oracle's records with the Gaussians in culled marked as having no record: what the
    4D preprocess is to leave (key 0xFFFFFFFF, no tiles)."""
    w = want.copy()
    w["status"][culled] = 0
    return w
