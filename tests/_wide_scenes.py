"""Scenes of large, tilted and clipped splats — TEST INFRASTRUCTURE.

gsr_synth_write_ply's splats are a few pixels wide and the hand-made dense scenes carry
the identity quaternion, so neither reaches the conservative shortcuts of the forward path
where they could be wrong: tile rects wider than six tiles or taller than four tile rows,
tilted ellipses whose edge crosses many 8x8 blocks, centres thousands of pixels off screen,
boxes that end at W or H, conics that are not robustly positive definite.  The scenes
below do (tests/test_wide_scenes.py asserts it on the oracle's records alone); they are a
few hundred Gaussians each, seen at 320x240 through test_gpu_parity.CAMS.

Every builder returns a (38, n) float32 array for Scene.from_soa and the oracle alike.
One generator per scene, drawn in this order: x, y, z; opacity; the three scales; the
quaternion (not normalised); the 27 SH values."""
from __future__ import annotations

import numpy as np

W, H = 320, 240

# name: n, seed, scales (lo, hi), opacity (lo, hi), box (x, y, z).  Opacities above 0.99
# clamp; opacities just above 1e-3 make the blend's md2 cut nearly 0.
SCENES = {
    "slabs": (256, 5, (0.01, 0.6), (0.002, 1.2), (3.0, 1.7, 1.0)),
    "needles": (256, 6, (0.0005, 0.8), (0.002, 1.2), (3.0, 1.7, 1.0)),
    "stack": (384, 9, (0.15, 0.9), (0.5, 1.5), (3.0, 1.7, 1.0)),
    "huge": (64, 7, (0.5, 5.0), (0.002, 1.2), (8.0, 8.0, 8.0)),
    "tilted": (200, 41, (0.02, 0.5), (0.01, 1.2), (0.5, 0.5, 0.5)),
}
GRAZE_SEEDS = (0, 1, 2, 3)


def _log_uniform(rng, lo, hi, size):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), size))


def _fill(rng, soa, scales, opacity):
    """Everything after the positions, in the documented order."""
    n = soa.shape[1]
    soa[3] = _log_uniform(rng, *opacity, n)
    soa[4:7] = _log_uniform(rng, *scales, (3, n))
    soa[7:11] = rng.standard_normal((4, n))
    soa[11:38] = rng.normal(0, 0.3, (27, n))
    return soa


def build(n, seed, scales, opacity, box):
    rng = np.random.default_rng(seed)
    soa = np.zeros((38, n), np.float32)
    for axis, b in enumerate(box):
        soa[axis] = rng.uniform(-b, b, n)
    return _fill(rng, soa, scales, opacity)


def scene(name, n=None, scales=None):
    """A scene of SCENES by name; n and scales override the table (the 8-bit digit frame's
    48-Gaussian `slabs`)."""
    n0, seed, s, op, box = SCENES[name]
    return build(n or n0, seed, scales or s, op, box)


def graze(seed, n=512):
    """Splats within 0.02 .. 1 world units in front of the default camera at (0, 0, 4): they
    graze the near plane, so their centres project up to +-15,000 pixels off the frame while
    their boxes still reach it."""
    rng = np.random.default_rng(seed)
    soa = np.zeros((38, n), np.float32)
    soa[0] = rng.uniform(-6.0, 6.0, n)
    soa[1] = rng.uniform(-6.0, 6.0, n)
    soa[2] = 4.0 - _log_uniform(rng, 0.02, 1.0, n)
    return _fill(rng, soa, (0.05, 3.0), (0.002, 1.2))


def unit_opacity(soa):
    """The scene with its opacities capped at 1.  The fast-exp blend's error bound assumes an
    opacity in [0, 1], so it hands every block that holds a record above 1 to the exact blend:
    on the scenes as drawn that is a third of slabs' blocks and every block of stack.  Capped,
    the fast blend's own arithmetic runs on these splats (opacity 1 still clamps at 0.99)."""
    s = soa.copy()
    s[3] = np.minimum(s[3], np.float32(1.0))
    return s


def rect_pairs(want, order, W, H):
    """test_gpu_parity.rect_pairs without its Python loop over every tile: (tile << 32 |
    index) for every tile of every visible splat's tile rect, stable by tile over the depth
    order."""
    tx, ty = (W + 15) // 16, (H + 15) // 16
    idx = (order & np.uint64(0xFFFFFFFF)).astype(np.int64)
    idx = idx[want["status"][idx] == 2]
    a = want["aabb"][idx].astype(np.int64)
    x0, x1 = a[:, 0] // 16, np.minimum(tx - 1, a[:, 2] // 16)
    y0, y1 = a[:, 1] // 16, np.minimum(ty - 1, a[:, 3] // 16)
    w = np.maximum(x1 - x0 + 1, 0)
    cnt = w * np.maximum(y1 - y0 + 1, 0)
    rep = np.repeat(np.arange(idx.size), cnt)
    j = np.arange(rep.size) - np.repeat(np.cumsum(cnt) - cnt, cnt)     # position in its rect, row-major
    tile = (y0[rep] + j // w[rep]) * tx + x0[rep] + j % w[rep]
    pairs = (tile.astype(np.uint64) << np.uint64(32)) | idx[rep].astype(np.uint64)
    return pairs[np.argsort(tile, kind="stable")]


def tile_rects(want, W, H):
    """(tx0, tx1, ty0, ty1) of the visible records' tile rects, from the oracle's aabb."""
    tx, ty = (W + 15) // 16, (H + 15) // 16
    a = want["aabb"][want["status"] == 2].astype(np.int64)
    return a[:, 0] // 16, np.minimum(tx - 1, a[:, 2] // 16), a[:, 1] // 16, np.minimum(ty - 1, a[:, 3] // 16)


def alpha_plane(orc, soa, cam, W, H, k):
    """The oracle's accumulated alpha: its image of the scene recoloured to exactly 1.0
    (f_rest zeroed, f_dc = 4 clamps to 1), the recolouring test_gpu_contrib.ones_soa uses."""
    s = soa.copy()
    s[14:38] = 0.0
    s[11] = 4.0
    return orc.render(s, cam, W, H, k)[0].copy()
