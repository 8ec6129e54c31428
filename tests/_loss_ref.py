"""The yardstick of gsr_image_loss's tests: the definition of include/gsr.h "image loss" written
with torch on the CPU, in float64 (the yardstick) or float32 (what single precision alone
costs), with the gradient from autograd; and the table of cases the tests share.

    L = w_l1 mean|x - y| + w_l2 mean (x - y)^2 + w_dssim (1 - mean SSIM(x, y))

SSIM per channel and pixel from five 11 x 11 Gaussian-windowed means (sigma 1.5, zero padding,
no renormalisation at the border), as 3DGS's ssim() computes it with conv2d(padding=5,
groups=3).  Images are planar (3, H, W); the window is symmetric, so the row order is free."""
import functools

import numpy as np
import torch

C1, C2 = 1e-4, 9e-4
RADIUS = 5
NVALUES = 4


def window1d():
    """g_k, k = 0..10: computed in double, normalised to sum 1, rounded to float32."""
    k = np.arange(2 * RADIUS + 1, dtype=np.float64)
    g = np.exp(-(k - RADIUS) ** 2 / (2 * 1.5 ** 2))
    return (g / g.sum()).astype(np.float32)


def _windowed(img, g):
    """The windowed mean of every (3, H, W) plane, zero padded: the separable window as
    eleven shifted multiply-adds along x, then eleven along y.  Plain elementwise operations
    in a fixed order, so a precision's result does not depend on a convolution library."""
    _, H, W = img.shape
    p = torch.nn.functional.pad(img, (RADIUS, RADIUS, RADIUS, RADIUS))
    h = sum(g[k] * p[:, :, k:k + W] for k in range(2 * RADIUS + 1))
    return sum(g[k] * h[:, k:k + H, :] for k in range(2 * RADIUS + 1))


def _mean(t):
    """The mean over every element as a balanced tree of elementwise additions (a fixed order,
    whatever the host's vector width)."""
    v = t.reshape(-1)
    n = v.numel()
    size = 1 << max(0, (n - 1).bit_length())
    v = torch.nn.functional.pad(v, (0, size - n))
    while v.numel() > 1:
        half = v.numel() // 2
        v = v[:half] + v[half:]
    return v[0] / n


def ssim_map(x, y):
    g = torch.from_numpy(window1d()).to(x.dtype)
    mu1, mu2 = _windowed(x, g), _windowed(y, g)
    s11 = _windowed(x * x, g) - mu1 * mu1
    s22 = _windowed(y * y, g) - mu2 * mu2
    s12 = _windowed(x * y, g) - mu1 * mu2
    return ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s11 + s22 + C2))


def loss_values(x, y, weights):
    """The four values of d_loss as a tensor {L, mean|d|, mean d^2, mean SSIM} (x, y: torch)."""
    d = x - y
    l1, l2, s = _mean(d.abs()), _mean(d * d), _mean(ssim_map(x, y))
    w1, w2, ws = weights
    return torch.stack([w1 * l1 + w2 * l2 + ws * (1 - s), l1, l2, s])


def evaluate(x, y, weights, dtype=torch.float64):
    """(values (4,), dL/dx (3, H, W)) as float64 numpy arrays, computed in `dtype`.  x and y are
    float32 numpy images: both precisions start from the same bits."""
    xt = torch.from_numpy(np.array(x, np.float32)).to(dtype).requires_grad_(True)
    yt = torch.from_numpy(np.array(y, np.float32)).to(dtype)
    vals = loss_values(xt, yt, weights)
    vals[0].backward()
    return vals.detach().numpy().astype(np.float64), xt.grad.numpy().astype(np.float64)


# ---------------------------------------------------------------- the case table

# W x H: one pixel; the window's width; either side of the 16-pixel tile; tile + both halos;
# wide and flat (the window taller than the image); one row over many tiles; odd sizes over
# several tiles in both directions; more workgroups than one wave of tiles.
SIZES = [(1, 1), (11, 11), (15, 15), (16, 16), (17, 17), (26, 26), (70, 5), (300, 1), (37, 29), (130, 33)]
CONTENTS = ("rand", "close", "bright", "zero", "equal")
WEIGHTINGS = [(0.8, 0.0, 0.2), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)]


def make_images(content, W, H):
    """(x, y) float32 (3, H, W), seeded by the case.
    rand: independent uniform x and y.  close: y uniform, x = y + N(0, 0.02).  bright: y in
    [0.98, 0.99], x = y + N(0, 0.005), a saturated render, the worst case for the E[x^2] - mu^2
    cancellation.  zero: rand with both images 0 in rows [0, H/2), pixels no splat reaches.
    equal: x = y."""
    rng = np.random.default_rng(1000 * CONTENTS.index(content) + 7 * W + H)
    shape = (3, H, W)
    if content == "rand":
        x, y = rng.random(shape), rng.random(shape)
    elif content == "close":
        y = rng.random(shape)
        x = y + rng.normal(0, 0.02, shape)
    elif content == "bright":
        y = rng.uniform(0.98, 0.99, shape)
        x = y + rng.normal(0, 0.005, shape)
    elif content == "zero":
        x, y = rng.random(shape), rng.random(shape)   # rows [0, H/2): no splat reached them
        x[:, :H // 2] = 0
        y[:, :H // 2] = 0
    elif content == "equal":
        y = rng.random(shape)
        x = y.copy()
    else:
        raise KeyError(content)
    return x.astype(np.float32), y.astype(np.float32)


CASES = {f"{c}-{W}x{H}": (c, W, H) for c in CONTENTS for (W, H) in SIZES}


@functools.lru_cache(maxsize=None)
def reference(case, weights):
    """The float64 yardstick of a case and weighting, computed once and shared: a dict of x, y
    (float32), values (4,), grad (3, H, W) and A = max|grad| (read-only arrays)."""
    content, W, H = CASES[case]
    x, y = make_images(content, W, H)
    vals, grad = evaluate(x, y, weights)
    out = dict(x=x, y=y, values=vals, grad=grad, A=float(np.abs(grad).max()), W=W, H=H, content=content)
    for a in (x, y, vals, grad):
        a.setflags(write=False)
    return out
