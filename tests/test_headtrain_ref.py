"""Pins tests/headtrain_ref.py, the float64 checker of the classifier head's
training mode (CPU only): a hand-computed BN case, gradcheck of the head,
agreement with oracle/heads_ref in inference mode, MaxNorm known answers."""
import math

import numpy as np
import torch

import headtrain_ref as HT
from oracle import heads_ref as HR

D = torch.float64


def test_bn_hand_computed_3x4():
    """z 3x4, eps 1e-3.  Columns: (1,2,3) mean 2 var 2/3; (0,0,3) mean 1 var 2;
    (-1,1,0) mean 0 var 2/3; (2,2,2) mean 2 var 0."""
    z = torch.tensor([[1., 0., -1., 2.], [2., 0., 1., 2.], [3., 3., 0., 2.]], dtype=D)
    gamma = torch.tensor([1., 2., 0.5, 1.], dtype=D)
    beta = torch.tensor([0., -1., 0., 0.5], dtype=D)
    y, mean, var = HT.bn_train(z, gamma, beta, 1e-3, relu=True)
    assert torch.equal(mean, torch.tensor([2., 1., 0., 2.], dtype=D))
    assert torch.allclose(var, torch.tensor([2 / 3, 2., 2 / 3, 0.], dtype=D), rtol=0, atol=1e-15)
    r0, r1, r3 = 1 / math.sqrt(2 / 3 + 1e-3), 1 / math.sqrt(2 + 1e-3), 1 / math.sqrt(1e-3)
    want = torch.tensor([[0., 0., 0., 0.5],                       # relu(-r0), relu(-2 r1 - 1), relu(-0.5 r0)
                         [0., 0., 0.5 * r0, 0.5],
                         [r0, 4 * r1 - 1, 0., 0.5]], dtype=D)     # column 3: (2 - 2) * r3 + 0.5
    assert torch.allclose(y, want, rtol=0, atol=1e-14)
    assert r3 > 31                                                # the zero-variance column is finite
    # moving statistics from (0, 1) with momentum 0.9: the correction is M/(M - 1.001) = 3/1.999
    mm, mv = HT.moving_update(torch.zeros(4, dtype=D), torch.ones(4, dtype=D), mean, var, 3, 0.9, 1e-3)
    assert torch.allclose(mm, torch.tensor([0.2, 0.1, 0., 0.2], dtype=D), rtol=0, atol=1e-15)
    k = 3 / 1.999
    assert torch.allclose(mv, torch.tensor([0.9 + (2 / 3) * k * 0.1, 0.9 + 2 * k * 0.1, 0.9 + (2 / 3) * k * 0.1,
                                            0.9], dtype=D), rtol=0, atol=1e-14)
    # backward, ReLU on.  Column 0: xhat = (-r0, 0, r0), y = (-r0, 0, r0) -> mask (0, 0, 1);
    # dy (1, 2, 4) -> dpre (0, 0, 4), dbeta 4, dgamma 4 r0,
    # dz = r0 * (dpre - 4/3 - xhat * 4 r0 / 3)
    dy = torch.tensor([[1., 1., 1., 1.], [2., 1., 1., 1.], [4., 1., 1., 1.]], dtype=D)
    dz, dgamma, dbeta = HT.bn_train_bwd(dy, y, z, gamma, mean, var, 1e-3, relu=True)
    assert abs(float(dbeta[0]) - 4.0) < 1e-14 and abs(float(dgamma[0]) - 4 * r0) < 1e-14
    want0 = [r0 * (0 - 4 / 3 + r0 * 4 * r0 / 3), r0 * (0 - 4 / 3), r0 * (4 - 4 / 3 - r0 * 4 * r0 / 3)]
    assert torch.allclose(dz[:, 0], torch.tensor(want0, dtype=D), rtol=0, atol=1e-13)
    # column 3 (constant z): xhat = 0, all rows pass the ReLU (y = 0.5): dbeta 3, dgamma 0,
    # dz = r3 * (1 - 3/3) = 0
    assert abs(float(dbeta[3]) - 3.0) < 1e-14 and float(dgamma[3]) == 0.0
    assert float(dz[:, 3].abs().max()) < 1e-13
    # ReLU off, column 1: xhat = (-r1, -r1, 2 r1), dpre = dy = 1: dbeta 3, dgamma 0, dz 0
    dz, dgamma, dbeta = HT.bn_train_bwd(dy, None, z, gamma, mean, var, 1e-3, relu=False)
    assert abs(float(dbeta[1]) - 3.0) < 1e-14 and abs(float(dgamma[1])) < 1e-14
    assert float(dz[:, 1].abs().max()) < 1e-13
    # ... and the closed form is autograd's
    zz = z.clone().requires_grad_(True)
    g2, b2 = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    yy, _, _ = HT.bn_train(zz, g2, b2, 1e-3, relu=True)
    (yy * dy).sum().backward()
    dz, dgamma, dbeta = HT.bn_train_bwd(dy, y, z, gamma, mean, var, 1e-3, relu=True)
    assert torch.allclose(zz.grad, dz, rtol=0, atol=1e-12)
    assert torch.allclose(g2.grad, dgamma, rtol=0, atol=1e-12) and torch.allclose(b2.grad, dbeta, rtol=0, atol=1e-12)


def small_params(pool, C, fc, nc, seed, dtype=D, moving=False):
    g = torch.Generator().manual_seed(seed)
    K = pool ** 3 * C

    def rn(*s, scale=1.0):
        return (torch.randn(*s, generator=g, dtype=torch.float64) * scale).to(dtype)
    p = {"mrcnn_class_conv1/kernel:0": rn(pool, pool, pool, C, fc, scale=1 / math.sqrt(K)),
         "mrcnn_class_conv1/bias:0": rn(fc, scale=0.1),
         "mrcnn_class_bn1/gamma:0": (rn(fc, scale=0.2) + 1.0), "mrcnn_class_bn1/beta:0": rn(fc, scale=0.3),
         "mrcnn_class_conv2/kernel:0": rn(1, 1, 1, fc, fc, scale=1 / math.sqrt(fc)),
         "mrcnn_class_conv2/bias:0": rn(fc, scale=0.1),
         "mrcnn_class_bn2/gamma:0": (rn(fc, scale=0.2) + 1.0), "mrcnn_class_bn2/beta:0": rn(fc, scale=0.3),
         "mrcnn_class_logits/kernel:0": rn(fc, nc, scale=0.5), "mrcnn_class_logits/bias:0": rn(nc, scale=0.1),
         "mrcnn_bbox_fc/kernel:0": rn(fc, 6 * nc, scale=0.3), "mrcnn_bbox_fc/bias:0": rn(6 * nc, scale=0.1)}
    if moving:
        for i in (1, 2):
            p[f"mrcnn_class_bn{i}/moving_mean:0"] = rn(fc, scale=0.2)
            p[f"mrcnn_class_bn{i}/moving_variance:0"] = (torch.rand(fc, generator=g, dtype=torch.float64) + 0.5).to(dtype)
    return p


def test_head_gradcheck_float64():
    pool, C, fc, nc = 2, 2, 4, 2
    p = small_params(pool, C, fc, nc, seed=5)
    g = torch.Generator().manual_seed(6)
    pooled = torch.randn(1, 6, pool, pool, pool, C, generator=g, dtype=D)
    names = list(HT.PARAM_NAMES)

    def fn(x, *ts):
        logits, _, bbox, _ = HT.head_forward(dict(zip(names, ts)), x, nc, training=True)
        return logits, bbox
    # away from the ReLU kinks and the clip bounds, or finite differences straddle them
    _, _, _, aux = HT.head_forward(p, pooled, nc, training=True)
    inputs = [pooled.requires_grad_(True)] + [p[k].clone().requires_grad_(True) for k in names]
    assert min(float(aux["pre1"].abs().min()), float(aux["pre2"].abs().min())) > 1e-4
    assert float(aux["raw_logits"].abs().max()) < 9.9
    assert torch.autograd.gradcheck(fn, inputs, eps=1e-6, atol=1e-6, rtol=1e-5)


def test_clip_gradient_is_zero_outside():
    pool, C, fc, nc = 2, 2, 4, 2
    p = small_params(pool, C, fc, nc, seed=7)
    p["mrcnn_class_logits/bias:0"] = torch.tensor([30.0, -30.0], dtype=D)       # every raw logit beyond +-10
    pooled = torch.randn(1, 5, pool, pool, pool, C, generator=torch.Generator().manual_seed(8), dtype=D)
    q = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    logits, _, _, aux = HT.head_forward(q, pooled, nc, training=True)
    assert float(aux["raw_logits"].detach().abs().min()) > 10.0
    assert set(logits.detach().unique().tolist()) == {-10.0, 10.0}
    (logits * torch.arange(10, dtype=D).reshape(1, 5, 2)).sum().backward()
    assert float(q["mrcnn_class_logits/kernel:0"].grad.abs().max()) == 0.0


def test_inference_mode_matches_the_oracle_head():
    pool, C, fc, nc = 3, 4, 8, 3
    p = small_params(pool, C, fc, nc, seed=9, moving=True)
    pooled = torch.randn(2, 5, pool, pool, pool, C, generator=torch.Generator().manual_seed(10), dtype=D)
    logits, probs, bbox, _ = HT.head_forward(p, pooled, nc, training=False)
    rl, rp, rb = HR.classifier_head({k: v.numpy() for k, v in p.items()}, pooled.numpy(), nc)
    for got, ref in ((logits, rl), (probs, rp), (bbox, rb)):
        assert got.shape == ref.shape
        assert float((got - ref).abs().max()) < 1e-12 * max(1.0, float(ref.abs().max()))


def test_max_norm_known_answers():
    w = torch.tensor([[0.6, 3.0, 0.0], [0.8, 4.0, 0.0]], dtype=D)
    out = HT.max_norm(w, 2.0)
    # under the bound (norm 1): shrinks only by the 1e-7 term; over it (norm 5): to 2; zero column stays 0
    assert torch.allclose(out[:, 0], w[:, 0] * (1.0 / (1.0 + 1e-7)), rtol=0, atol=1e-16)
    assert float(out[:, 0].norm()) < 1.0 and float(out[:, 0].norm()) > 1.0 - 2e-7
    assert torch.allclose(out[:, 1], w[:, 1] * (2.0 / (5.0 + 1e-7)), rtol=0, atol=1e-16)
    assert abs(float(out[:, 1].norm()) - 2.0) < 1e-7
    assert torch.equal(out[:, 2], torch.zeros(2, dtype=D)) and bool(torch.isfinite(out).all())


def test_train_steps_apply_the_constraint_and_the_l2_term():
    pool, C, fc, nc = 2, 2, 4, 2
    p = small_params(pool, C, fc, nc, seed=11)
    p["mrcnn_bbox_fc/kernel:0"] = p["mrcnn_bbox_fc/kernel:0"] * 10.0               # column norms above 1
    g = torch.Generator().manual_seed(12)
    pooled = torch.randn(1, 8, pool, pool, pool, C, generator=g, dtype=D)
    ids = torch.tensor([[1, 0, 1, 0, 1, 0, 0, 0]])
    tb = torch.randn(1, 8, 6, generator=g, dtype=D)
    active = torch.ones(1, nc, dtype=D)
    mov = {f"bn{i}": (torch.zeros(fc, dtype=D), torch.ones(fc, dtype=D)) for i in (1, 2)}
    traj, q, mov2 = HT.train_steps(p, mov, pooled, ids, tb, active, nc, 3, ("SGD", 0.05, 0.9), weight_decay=0.1)
    assert traj.shape == (3, 4) and np.isfinite(traj).all()
    assert float(q["mrcnn_bbox_fc/kernel:0"].norm(dim=0).max()) <= 1.0
    assert float(q["mrcnn_class_logits/kernel:0"].norm(dim=0).max()) <= 2.0
    assert not torch.equal(mov2["bn1"][0], mov["bn1"][0])
    # the l2 term moves a parameter whose loss gradient is zero (conv biases under batch statistics)
    _, q0, _ = HT.train_steps(p, mov, pooled, ids, tb, active, nc, 1, ("SGD", 0.05, 0.0), weight_decay=0.0)
    _, q1, _ = HT.train_steps(p, mov, pooled, ids, tb, active, nc, 1, ("SGD", 0.05, 0.0), weight_decay=0.1)
    b = "mrcnn_class_conv1/bias:0"
    assert float((q0[b] - p[b]).abs().max()) < 1e-12
    assert torch.allclose(q1[b] - p[b], -0.05 * (0.1 / fc) * p[b], rtol=0, atol=1e-12)
