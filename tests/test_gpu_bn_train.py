"""Batch-statistics BatchNorm (m3d_bn_train_fwd / m3d_bn_train_bwd through
m3d.heads.bn_train_fwd / bn_train_bwd) against the float64 CPU evaluation of
tests/headtrain_ref.py (pinned by tests/test_headtrain_ref.py): y, the saved
mean / rstd, the moving statistics after two consecutive forwards, dz, dgamma
and dbeta, every element compared, with and without the ReLU.

Shapes (M, C): (2, 4) the smallest legal one; (37, 36) nothing a multiple of
the tile; (128, 512) the classifier head's regime at a real width; (1440, 32)
rows = 8 ROIs x 6x6x5 voxels; FEW and FEW + 1 rows x 20 channels on either side
of M3D_BN_TRAIN_FEW_ROWS_MAX (one workgroup per strip / per-row-block
partials).  Also on every shape: y aliasing z, dz aliasing dy, dgamma / dbeta
added onto non-zero destinations, NULL moving pointers, two runs bit-identical,
forward + backward captured in a HIP graph and replayed equal to eager.

Inputs: z = N(mu_c, s_c) per column, s_c in [0.5, 2]; every column's batch
variance is raised to >= 1e-2 if it fell below (the BN gradient is
ill-conditioned below eps); an entry whose float64 pre-activation gamma xhat +
beta lies within 1e-4 of 0 is resampled (never dropped), so the float32 kernel
and the checker take the same ReLU branch.

Bars: tensors relative to the reference tensor's largest entry.  Per shape and
quantity, 10x the worst error (ReLU on and off) of the restatement evaluated
in float32 on the CPU against float64 (scripts/measure_headtrain_f32.py prints
the table F32 below) -- room for another summation order, not for a wrong
term -- but never below 1e-6 = 16 float32 ulps of the scale: each quantity goes
through about that many float32 roundings, and the worst of a shape's few
channels (4 at the smallest) under-samples them.  Measured float32 errors are
0.2e-7..2e-7 everywhere except y (7e-7) and dz (1.3e-5) at M = 2, where xhat
= +-1 and dz cancels to about 0; so every bar is 1e-6..1.9e-6 except those two
(7.2e-6, 1.3e-4).  Measured on an MI355X: 0.4e-7..2.4e-7 for every quantity
and shape, except at M = 2 y 7.2e-7, moving_mean 3.9e-7 and dz 1.3e-5 -- the
float32 figures themselves.
"""
import functools
import types

import numpy as np
import pytest
import torch

import headtrain_ref as HT

pytestmark = pytest.mark.gpu

FEW = 2048                       # M3D_BN_TRAIN_FEW_ROWS_MAX (asserted against the library below)
SHAPES = [(2, 4), (37, 36), (128, 512), (8 * 6 * 6 * 5, 32), (FEW, 20), (FEW + 1, 20)]
MOMENTUM, EPS = 0.9, 1e-3
QUANTITIES = ("y", "mean", "rstd", "mm", "mv", "dz", "dgamma", "dbeta")
# worst float32-vs-float64 error of the restatement on the CPU per shape, ReLU on and off
# (scripts/measure_headtrain_f32.py); each bar is 10x its figure
F32 = {
    (2, 4): (7.15e-07, 3.43e-08, 2.28e-08, 5.09e-08, 1.20e-07, 1.34e-05, 2.09e-07, 4.03e-08),
    (37, 36): (1.21e-07, 1.01e-07, 5.58e-08, 7.23e-08, 9.00e-08, 1.33e-07, 1.88e-07, 8.81e-08),
    (128, 512): (1.53e-07, 9.14e-08, 1.03e-07, 1.04e-07, 1.14e-07, 1.16e-07, 1.89e-07, 1.04e-07),
    (1440, 32): (1.75e-07, 5.10e-08, 8.57e-08, 7.35e-08, 1.13e-07, 1.14e-07, 1.90e-07, 1.10e-07),
    (FEW, 20): (1.67e-07, 6.12e-08, 5.75e-08, 6.95e-08, 1.85e-07, 8.64e-08, 1.24e-07, 1.57e-07),
    (FEW + 1, 20): (1.41e-07, 5.58e-08, 6.29e-08, 1.15e-07, 6.04e-08, 1.39e-07, 1.63e-07, 1.13e-07),
}
FLOOR = 1e-6          # 16 float32 ulps of the scale: no bar below the format's own rounding (see docstring)
BARS = {shape: {k: max(10.0 * v, FLOOR) for k, v in zip(QUANTITIES, row)} for shape, row in F32.items()}
CASES = [(M, C, relu) for (M, C) in SHAPES for relu in (True, False)]


@functools.lru_cache(maxsize=None)
def case(M, C, relu, seed=0):
    """float32 host inputs of one shape and their float64 reference."""
    rng = np.random.default_rng(seed + 1000 * M + C)
    mu, sd = rng.normal(0, 1, C), rng.uniform(0.5, 2.0, C)
    z = (mu + sd * rng.normal(size=(M, C))).astype(np.float32)
    gamma = rng.uniform(0.5, 1.5, C).astype(np.float32)
    beta = rng.normal(0, 0.3, C).astype(np.float32)
    for _ in range(50):
        z64 = z.astype(np.float64)
        var = z64.var(0)
        low = var < 1e-2
        if low.any():                       # spread the column about its mean (M = 2 can draw two close values)
            m = z64.mean(0)
            k = np.where(low, 1.5 * np.sqrt(1e-2 / np.maximum(var, 1e-30)), 1.0)
            z = (m + (z64 - m) * k).astype(np.float32)
            continue
        pre = gamma * (z64 - z64.mean(0)) / np.sqrt(var + EPS) + beta
        bad = np.abs(pre) < 1e-4
        if not bad.any():
            break
        z[bad] = (mu + sd * rng.normal(size=(M, C))).astype(np.float32)[bad]
    dy = rng.normal(size=(M, C)).astype(np.float32)
    g0 = rng.normal(size=(2, C)).astype(np.float32)            # non-zero dgamma / dbeta destinations
    mm0 = rng.normal(0, 0.2, C).astype(np.float32)
    mv0 = rng.uniform(0.5, 1.5, C).astype(np.float32)
    return dict(z=z, gamma=gamma, beta=beta, dy=dy, g0=g0, mm0=mm0, mv0=mv0)


def reference(c, relu, dtype=torch.float64):
    t = {k: torch.from_numpy(v).to(dtype) for k, v in c.items()}
    M = t["z"].shape[0]
    y, mean, var = HT.bn_train(t["z"], t["gamma"], t["beta"], EPS, relu)
    pre, _, _ = HT.bn_train(t["z"], t["gamma"], t["beta"], EPS, False)
    mm, mv = HT.moving_update(t["mm0"], t["mv0"], mean, var, M, MOMENTUM, EPS)
    mm, mv = HT.moving_update(mm, mv, mean, var, M, MOMENTUM, EPS)          # two consecutive forwards
    dz, dgamma, dbeta = HT.bn_train_bwd(t["dy"], y, t["z"], t["gamma"], mean, var, EPS, relu)
    return dict(y=y, mean=mean, rstd=1.0 / torch.sqrt(var + EPS), mm=mm, mv=mv, dz=dz,
                dgamma=t["g0"][0] + dgamma, dbeta=t["g0"][1] + dbeta, pre=pre, var=var)


def rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.double()
    return float((got - ref).abs().max()) / float(ref.abs().max())


def _bn(c, dev):
    """A BNLayer-shaped object on the device (gamma/beta with gradient views,
    moving statistics, eps, momentum)."""
    d = {k: torch.from_numpy(v).to(dev) for k, v in c.items()}
    bn = types.SimpleNamespace(eps=EPS, momentum=MOMENTUM, moving_mean=d["mm0"].clone(),
                               moving_variance=d["mv0"].clone(),
                               gamma=types.SimpleNamespace(data=d["gamma"], grad=d["g0"][0].clone()),
                               beta=types.SimpleNamespace(data=d["beta"], grad=d["g0"][1].clone()))
    return d, bn


def test_cases_meet_their_preconditions():
    from m3d.heads import bn_train_few_rows_max
    assert bn_train_few_rows_max() == FEW
    for M, C, relu in CASES:
        r = reference(case(M, C, relu), relu)
        assert float(r["var"].min()) >= 1e-2, (M, C)
        assert float(r["pre"].abs().min()) >= 1e-4, (M, C)


@pytest.mark.parametrize("M,C,relu", CASES)
def test_forward_backward_match_float64(cuda, M, C, relu):
    from m3d.heads import bn_train_bwd, bn_train_fwd
    c = case(M, C, relu)
    r = reference(c, relu)
    d, bn = _bn(c, cuda)
    y, mean, rstd = bn_train_fwd(d["z"], bn, relu)
    y_b, mean_b, rstd_b = bn_train_fwd(d["z"], bn, relu)          # second forward: moving statistics move again
    dz = bn_train_bwd(d["dy"], y, d["z"], bn, mean, rstd, relu)
    got = dict(y=y, mean=mean, rstd=rstd, mm=bn.moving_mean, mv=bn.moving_variance, dz=dz, dgamma=bn.gamma.grad,
               dbeta=bn.beta.grad)
    bars = BARS[(M, C)]
    errs = {k: rel(got[k], r[k]) for k in QUANTITIES}
    print(f"bn_train M={M} C={C} relu={int(relu)} " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    for k, bar in bars.items():
        assert errs[k] <= bar, (k, errs[k], bar)
    assert torch.equal(y, y_b) and torch.equal(mean, mean_b) and torch.equal(rstd, rstd_b)
    # y aliasing z
    z2 = d["z"].clone()
    y_alias, _, _ = bn_train_fwd(z2, bn, relu, y=z2, update_moving=False)
    assert y_alias.data_ptr() == z2.data_ptr() and torch.equal(y_alias, y)
    # dz aliasing dy (dgamma / dbeta accumulate a second time onto the first result)
    g1, b1 = bn.gamma.grad.clone(), bn.beta.grad.clone()
    dy2 = d["dy"].clone()
    dz_alias = bn_train_bwd(dy2, y, d["z"], bn, mean, rstd, relu, dz=dy2)
    assert dz_alias.data_ptr() == dy2.data_ptr() and torch.equal(dz_alias, dz)
    g0 = torch.from_numpy(c["g0"]).double()
    twice = dict(dgamma=2 * r["dgamma"] - g0[0], dbeta=2 * r["dbeta"] - g0[1])
    for k, got2 in (("dgamma", bn.gamma.grad), ("dbeta", bn.beta.grad)):
        err = float((got2.double().cpu() - twice[k]).abs().max())
        assert err <= bars[k] * float(r[k].abs().max() + twice[k].abs().max()), (k, err)
    assert not torch.equal(bn.gamma.grad, g1) and not torch.equal(bn.beta.grad, b1)


@pytest.mark.parametrize("M,C,relu", CASES)
def test_null_moving_pointers_and_bit_identical_runs(cuda, M, C, relu):
    from m3d.heads import bn_train_bwd, bn_train_fwd
    c = case(M, C, relu)
    runs = []
    for _ in range(2):
        d, bn = _bn(c, cuda)
        y, mean, rstd = bn_train_fwd(d["z"], bn, relu, update_moving=False)
        assert torch.equal(bn.moving_mean, d["mm0"]) and torch.equal(bn.moving_variance, d["mv0"])
        y2, _, _ = bn_train_fwd(d["z"], bn, relu)
        dz = bn_train_bwd(d["dy"], y, d["z"], bn, mean, rstd, relu)
        runs.append((y, mean, rstd, y2, bn.moving_mean, bn.moving_variance, dz, bn.gamma.grad, bn.beta.grad))
    assert not torch.equal(runs[0][4], torch.from_numpy(c["mm0"]).to(cuda))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("M,C,relu", CASES)
def test_graph_capture_equals_eager(cuda, M, C, relu):
    from m3d.heads import bn_train_bwd, bn_train_fwd
    c = case(M, C, relu)
    d, bn = _bn(c, cuda)
    y, mean, rstd = bn_train_fwd(d["z"], bn, relu)
    dz = bn_train_bwd(d["dy"], y, d["z"], bn, mean, rstd, relu)
    eager = [t.clone() for t in (y, mean, rstd, dz, bn.moving_mean, bn.moving_variance, bn.gamma.grad, bn.beta.grad)]
    d2, bn2 = _bn(c, cuda)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gy, gmean, grstd = bn_train_fwd(d2["z"], bn2, relu)
        gdz = bn_train_bwd(d2["dy"], gy, d2["z"], bn2, gmean, grstd, relu)
    # capture runs nothing: restore the state the replay starts from, then replay once
    bn2.moving_mean.copy_(d2["mm0"]); bn2.moving_variance.copy_(d2["mv0"])
    bn2.gamma.grad.copy_(d2["g0"][0]); bn2.beta.grad.copy_(d2["g0"][1])
    graph.replay()
    torch.cuda.synchronize()
    got = (gy, gmean, grstd, gdz, bn2.moving_mean, bn2.moving_variance, bn2.gamma.grad, bn2.beta.grad)
    for a, b in zip(got, eager):
        assert torch.equal(a, b)
