"""The Adam twin (tests/_adam_ref.py) in float64 against torch.optim.Adam on the RAW parameters
— logit(opacity), log(scale), log(trbf_scale), the plain arrays as they are — with the same
betas, eps and learning rates as parameter groups, mapped back through sigmoid and exp.  The
two are the same mathematics in double; only the operation order and the logit / log round
trip differ, so they agree within 1e-10 relative.  This pins the twin's chain factors
(o (1 - o), s), its bias correction and where eps enters to an independent optimiser; the
GPU tests then pin the kernel to the twin bit for bit."""
import numpy as np
import pytest

import torch

import _adam_ref as ref

N, STEPS, RTOL = 257, 5, 1e-10
LRS = {"lr_position": 1.6e-4, "lr_opacity": 0.05, "lr_scale": 5e-3, "lr_rot": 1e-3, "lr_sh_dc": 2.5e-3,
       "lr_sh_rest": 1.25e-4, "lr_tcenter": 1e-4, "lr_tscale": 3e-3, "lr_motion": 2e-4}
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8   # an eps large enough that its place in the formula shows


def random_scene(narrays, n, rng):
    soa = np.zeros((narrays, n), np.float64)
    soa[0:3] = rng.uniform(-0.5, 0.5, (3, n))
    soa[3] = rng.uniform(0.05, 0.95, n)
    soa[4:7] = rng.uniform(0.05, 0.5, (3, n))
    soa[7:11] = rng.normal(0, 1, (4, n))
    sh_end = 59 if narrays == 59 else 38
    soa[11:sh_end] = rng.normal(0, 0.3, (sh_end - 11, n))
    if narrays == 49:
        soa[38] = rng.uniform(0, 1, n)
        soa[39] = rng.uniform(0.03, 0.15, n)
        soa[40:49] = rng.normal(0, 0.2, (9, n))
    return soa


def random_grads(narrays, n, rng):
    """Gradients with respect to the stored values, magnitudes over four decades."""
    return {k: rng.normal(0, 1, (p, n)) * 10.0 ** rng.uniform(-3, 1, (p, n))
            for k, p in ref.planes_of(narrays).items() if k != "temporal" or narrays == 49}


def close(a, b):
    return bool((np.abs(a - b) <= RTOL * np.maximum(np.abs(a), np.abs(b))).all())


@pytest.mark.parametrize("narrays", [38, 49, 59])
def test_twin_matches_torch_adam(narrays):
    rng = np.random.default_rng(narrays)
    soa = random_scene(narrays, N, rng)
    batches = [random_grads(narrays, N, rng) for _ in range(STEPS)]
    keys = list(batches[0])

    # torch: one raw parameter per group, one parameter group per learning rate
    raw, kinds, param_groups = [], [], []
    for key, first, planes, array, lr_key, kind in ref.groups(narrays):
        x = soa[array:array + planes]
        r = np.log(x / (1 - x)) if kind == ref.OPACITY else np.log(x) if kind == ref.EXP else x
        p = torch.tensor(r, dtype=torch.float64, requires_grad=True)
        raw.append(p)
        kinds.append((key, first, planes, array, kind))
        param_groups.append({"params": [p], "lr": LRS[lr_key]})
    opt = torch.optim.Adam(param_groups, betas=(BETA1, BETA2), eps=EPS)

    def stored(p, kind):
        with torch.no_grad():
            return (torch.sigmoid(p) if kind == ref.OPACITY else torch.exp(p) if kind == ref.EXP else p).numpy().copy()

    m = {k: np.zeros_like(batches[0][k]) for k in keys}
    v = {k: np.zeros_like(batches[0][k]) for k in keys}
    twin = soa.copy()
    for t, g in enumerate(batches, start=1):
        # the stored-value gradient carried to the raw parameter by torch's own autograd
        for p, (key, first, planes, array, kind) in zip(raw, kinds):
            act = torch.sigmoid(p) if kind == ref.OPACITY else torch.exp(p) if kind == ref.EXP else p
            p.grad = None
            (act * torch.tensor(g[key][first:first + planes])).sum().backward()
        opt.step()
        twin, _, m, v, bad = ref.adam_step(twin, g, m, v, LRS, t, np.exp, BETA1, BETA2, EPS)
        assert bad == 0 and twin.dtype == np.float64
        for p, (key, first, planes, array, kind) in zip(raw, kinds):
            assert close(twin[array:array + planes], stored(p, kind)), (t, key, first)
    # the moments are the raw-space moments
    for p, (key, first, planes, array, kind) in zip(raw, kinds):
        st = opt.state[p]
        assert close(m[key][first:first + planes], st["exp_avg"].numpy()), key
        assert close(v[key][first:first + planes], st["exp_avg_sq"].numpy()), key
    assert np.abs(twin - soa).max() > 1e-3   # the steps moved something


def test_twin_float32_is_float32(orc):
    """In float32 no operation of the twin is promoted, the exp is orc_expf, and skipped
    elements keep their bits."""
    rng = np.random.default_rng(1)
    n = 65
    soa = random_scene(38, n, rng).astype(np.float32)
    g = {k: a.astype(np.float32) for k, a in random_grads(38, n, rng).items()}
    g["opacity"][0, [0, 5]] = [np.nan, 0.0]
    g["scale"][2, n - 1] = -np.inf
    m = {k: np.zeros_like(a) for k, a in g.items()}
    v = {k: np.zeros_like(a) for k, a in g.items()}
    out, g2, m2, v2, bad = ref.adam_step(soa, g, m, v, LRS, 1, ref.orc_exp32(orc), skip_zero=True, zero_grads=True)
    assert out.dtype == np.float32 and all(a.dtype == np.float32 for a in (*m2.values(), *v2.values()))
    assert bad == 2
    assert out[3, 0] == soa[3, 0] and out[3, 5] == soa[3, 5] and out[6, n - 1] == soa[6, n - 1]
    assert m2["opacity"][0, 5] == 0 and v2["scale"][2, n - 1] == 0
    assert (out[3, 1:5] != soa[3, 1:5]).all()
    assert all(not a.any() for a in g2.values())
    # a frozen group is returned as it came
    out3, g3, _, _, _ = ref.adam_step(soa, g, m, v, {"lr_position": 1e-3}, 1, ref.orc_exp32(orc), zero_grads=True)
    assert np.array_equal(out3[3:], soa[3:]) and (out3[0:3] != soa[0:3]).any()
    assert not g3["position"].any() and np.array_equal(g3["rot"], g["rot"])
