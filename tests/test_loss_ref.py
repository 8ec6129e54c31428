"""The yardstick of gsr_image_loss's GPU tests (tests/_loss_ref.py), checked on the CPU: its
values against a brute-force per-pixel loop of the definition, its autograd gradient against
central differences of its own forward, the x == y case, and itself in float32 (E32 and EL32,
from which the GPU tolerances are taken)."""
import numpy as np
import pytest
import torch

import _loss_ref as lr


def brute_force(x, y):
    """(mean|d|, mean d^2, SSIM map) by the definition, one pixel and one window tap at a time,
    in Python floats (double): zero outside the image, the window not renormalised."""
    g = [float(v) for v in lr.window1d()]
    C, H, W = x.shape
    x, y = x.astype(np.float64), y.astype(np.float64)
    ssim = np.zeros((C, H, W))
    for c in range(C):
        for py in range(H):
            for px in range(W):
                mu1 = mu2 = e11 = e22 = e12 = 0.0
                for j in range(11):
                    qy = py + j - 5
                    if not 0 <= qy < H:
                        continue
                    for i in range(11):
                        qx = px + i - 5
                        if not 0 <= qx < W:
                            continue
                        w = g[j] * g[i]
                        a, b = x[c, qy, qx], y[c, qy, qx]
                        mu1 += w * a
                        mu2 += w * b
                        e11 += w * a * a
                        e22 += w * b * b
                        e12 += w * a * b
                s1, s2, s12 = e11 - mu1 * mu1, e22 - mu2 * mu2, e12 - mu1 * mu2
                ssim[c, py, px] = ((2 * mu1 * mu2 + lr.C1) * (2 * s12 + lr.C2)) / \
                                  ((mu1 * mu1 + mu2 * mu2 + lr.C1) * (s1 + s2 + lr.C2))
    d = x - y
    return np.abs(d).mean(), (d * d).mean(), ssim


def test_window():
    g = lr.window1d()
    assert g.dtype == np.float32 and g.shape == (11,)
    assert np.array_equal(g, g[::-1]) and g.argmax() == 5
    assert abs(float(g.astype(np.float64).sum()) - 1) < 1e-7
    assert abs(g[5] / g[4] - np.exp(1 / 4.5)) < 1e-6     # sigma = 1.5


@pytest.mark.parametrize("W,H", [(7, 9), (13, 12)])
def test_against_the_brute_force_loop(W, H):
    """Fixes the zero padding and the window: every window of a 7 x 9 image leaves the image,
    13 x 12 has windows that leave it on one side only and (one column) on neither."""
    for content in ("rand", "zero"):
        x, y = lr.make_images(content, W, H)
        l1, l2, ssim = brute_force(x, y)
        got = lr.ssim_map(torch.from_numpy(x).double(), torch.from_numpy(y).double()).numpy()
        assert np.abs(got - ssim).max() < 1e-13
        for w in lr.WEIGHTINGS:
            vals, _ = lr.evaluate(x, y, w)
            want = [w[0] * l1 + w[1] * l2 + w[2] * (1 - ssim.mean()), l1, l2, ssim.mean()]
            assert np.abs(vals - want).max() < 1e-13


@pytest.mark.parametrize("content", ["rand", "close", "bright", "zero"])
def test_gradient_against_central_differences(content):
    """Autograd against (L(x + h e) - L(x - h e)) / 2h in float64 at 24 elements of a 13 x 12
    image.  h = 1e-6: the truncation error h^2 L''' / 6 is far below the rounding error
    eps |L| / h <= 2.2e-16 / 1e-6 = 2.2e-10 of the difference, so 1e-8 bounds it with room (a
    gradient entry is about 1 / (3 W H) = 2e-3).  Elements within h of the L1 kink are left out."""
    W, H, h = 13, 12, 1e-6
    x, y = lr.make_images(content, W, H)
    x64 = x.astype(np.float64)
    rng = np.random.default_rng(5)
    yt = torch.from_numpy(y).double()
    for w in lr.WEIGHTINGS:
        _, grad = lr.evaluate(x, y, w)
        picks = [i for i in rng.permutation(x.size) if abs(x64.flat[i] - float(y.flat[i])) > 10 * h][:24]
        assert len(picks) == 24
        for i in picks:
            f = []
            for s in (+1, -1):
                xp = x64.copy()
                xp.flat[i] += s * h
                f.append(float(lr.loss_values(torch.from_numpy(xp), yt, w)[0]))
            assert abs((f[0] - f[1]) / (2 * h) - grad.flat[i]) < 1e-8, (w, i)


def test_equal_images():
    """x == y: SSIM is 1 everywhere, the L1 and L2 gradients are exactly 0 (sign(0) = 0) and
    the SSIM gradient is 0 up to float64 rounding through the 1 / C2 = 1.1e3 conditioning."""
    for case, (content, W, H) in lr.CASES.items():
        if content != "equal":
            continue
        for w in lr.WEIGHTINGS:
            r = lr.reference(case, w)
            assert np.array_equal(r["x"], r["y"])
            assert abs(r["values"][3] - 1) < 1e-12 and r["values"][1] == 0 and r["values"][2] == 0
            assert abs(r["values"][0]) < 1e-12
            assert r["A"] < 1e-12
            if w[2] == 0:
                assert r["A"] == 0


# What single precision alone costs: the reference evaluated in float32 against itself in
# float64, from the same float32 images.  E32[family]: the largest |g32 - g64| / A over the
# family's sizes and weightings, A = max|g64| of the case (a case whose float64 gradient is
# exactly zero has no scale: there the float32 gradient is not measured, and the GPU test asks
# for exactly zero).  EL32: the same for the four loss values, absolute.  The GPU tests allow 8 x
# these.  Measured: rand 5.79e-7, close 4.98e-6, bright 1.58e-4, zero 2.61e-7, equal 1.02e9 (the
# exact gradient of equal images is 0, so A is the float64 evaluation's own rounding residue,
# 1e-19 .. 1e-17, and the figure is the ratio of the two precisions' residues); EL32 2.29e-6.
E32 = {"rand": 6e-7, "close": 5e-6, "bright": 1.6e-4, "zero": 2.7e-7, "equal": 1.1e9}
EL32 = 2.3e-6


def test_float32_error_is_e32():
    worst = {c: 0.0 for c in lr.CONTENTS}
    worst_values = 0.0
    for case, (content, W, H) in lr.CASES.items():
        for w in lr.WEIGHTINGS:
            r = lr.reference(case, w)
            v32, g32 = lr.evaluate(r["x"], r["y"], w, torch.float32)
            worst_values = max(worst_values, float(np.abs(v32 - r["values"]).max()))
            if r["A"] > 0:
                worst[content] = max(worst[content], float(np.abs(g32 - r["grad"]).max()) / r["A"])
    print("E32", worst, "EL32", worst_values)
    for content in lr.CONTENTS:
        assert E32[content] / 2 <= worst[content] <= E32[content], content
    assert EL32 / 2 <= worst_values <= EL32
    # the families separate: the saturated render is the hard one
    assert E32["bright"] > 10 * E32["close"] > 50 * E32["rand"]


def test_case_table():
    assert len(lr.CASES) == len(lr.CONTENTS) * len(lr.SIZES) == 50
    assert set(lr.SIZES) == {(1, 1), (11, 11), (15, 15), (16, 16), (17, 17), (26, 26), (70, 5), (300, 1), (37, 29),
                             (130, 33)}
    assert lr.WEIGHTINGS == [(0.8, 0.0, 0.2), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)]
    x, y = lr.make_images("zero", 37, 29)
    assert not x[:, :14].any() and not y[:, :14].any() and x[:, 14:].all()
    x, y = lr.make_images("bright", 37, 29)
    assert y.min() >= 0.98 and y.max() <= 0.99
    assert lr.reference("rand-37x29", lr.WEIGHTINGS[0]) is lr.reference("rand-37x29", lr.WEIGHTINGS[0])
