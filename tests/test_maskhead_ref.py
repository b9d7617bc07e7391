"""Pins tests/maskhead_ref.py, the checker of the mask head's training mode
(no GPU): central finite differences in float64, hand-computed index maps of
the transposed conv and of the dilated taps, the BN shared with
tests/headtrain_ref.py, and the branch-agreement preconditions of
tests/test_gpu_mask_head_train.py on the float32 restatement."""
import pytest
import torch

import headtrain_ref as HT
import maskhead_ref as MR


def test_gradients_match_central_finite_differences():
    """Directional derivatives of the loss along a random direction of every
    parameter tensor and of pooled, eps = 1e-6 in float64."""
    c = MR.to(MR.case("tiny"))
    loss, grads, d_pooled, _, _ = MR.loss_and_grads(c["p"], c["pooled"], c["ids"], c["tmask"])
    g = torch.Generator().manual_seed(5)
    eps = 1e-6

    def value(p, pooled):
        with torch.no_grad():
            return float(MR.HL.mask_loss(c["tmask"], c["ids"], MR.forward(p, pooled)[0]))
    worst = 0.0
    for k in MR.PARAM_NAMES + ("pooled",):
        base = c["pooled"] if k == "pooled" else c["p"][k]
        d = torch.randn(base.shape, generator=g, dtype=torch.float64)
        vals = []
        for sgn in (1.0, -1.0):
            moved = base + sgn * eps * d
            vals.append(value(c["p"], moved) if k == "pooled" else value({**c["p"], k: moved}, c["pooled"]))
        fd = (vals[0] - vals[1]) / (2 * eps)
        an = float(((d_pooled if k == "pooled" else grads[k]) * d).sum())
        # the conv biases' derivative is 0 under batch statistics: absolute floor
        err = abs(fd - an) / max(abs(an), 1e-4)
        worst = max(worst, err)
        assert err < 2e-5, (k, fd, an)
    assert float(loss) > 0 and worst > 0


def test_conv_biases_have_zero_gradient_under_batch_statistics():
    c = MR.to(MR.case("tiny"))
    _, grads, _, _, aux = MR.loss_and_grads(c["p"], c["pooled"], c["ids"], c["tmask"])
    for conv, k in zip(MR.CONVS, MR.CONV_BIASES):
        dz = aux[f"z_{conv}"].grad
        assert float(grads[k].abs().max()) < 1e-12 * float(dz.abs().sum())
    assert float(grads["mrcnn_mask_deconv/bias:0"].abs().max()) > 1e-6


def test_deconv_index_map_known_answers():
    """x one-hot at voxel (1,0,2), channel 1 of [1,2,1,3,2]: y[2i+a, 2j+b, 2k+c, o]
    = w[a,b,c,o,1] + bias[o] on that voxel's 2^3 block, bias elsewhere."""
    w = torch.arange(2 * 2 * 2 * 3 * 2, dtype=torch.float64).reshape(2, 2, 2, 3, 2) + 1.0
    bias = torch.tensor([0.5, -1.0, 2.0], dtype=torch.float64)
    x = torch.zeros(1, 2, 1, 3, 2, dtype=torch.float64)
    x[0, 1, 0, 2, 1] = 1.0
    y = MR.deconv_k2s2(x, w, bias)
    assert tuple(y.shape) == (1, 4, 2, 6, 3)
    want = bias.expand(1, 4, 2, 6, 3).clone()
    for a in range(2):
        for b in range(2):
            for cc in range(2):
                want[0, 2 + a, 0 + b, 4 + cc] += w[a, b, cc, :, 1]
    assert torch.equal(y, want)
    assert float(y[0, 3, 1, 5, 2]) == 50.0          # by hand: w[1,1,1,2,1] = 24 + 12 + 6 + 4 + 1 + 1 = 48, + bias 2


def test_dilated_taps_known_answers():
    """p = 3, dilation 2: tap t reads x[o + 2(t - 1)], so only o = 0 <-> 2 and the
    centre tap are in range; o = 1 sees its own voxel alone."""
    w = torch.arange(27, dtype=torch.float64).reshape(3, 3, 3, 1, 1) + 1.0
    zero = torch.zeros(1, dtype=torch.float64)
    x = torch.zeros(1, 3, 3, 3, 1, dtype=torch.float64)
    x[0, 0, 0, 0, 0] = 1.0
    y = MR.conv_same(x, w, zero, 2)[0, ..., 0]
    want = torch.zeros(3, 3, 3, dtype=torch.float64)
    for a, oa in ((0, 2), (1, 0)):                   # tap index -> the output that reads voxel 0 through it
        for b, ob in ((0, 2), (1, 0)):
            for cc, oc in ((0, 2), (1, 0)):
                want[oa, ob, oc] = w[a, b, cc, 0, 0]
    assert torch.equal(y, want)
    assert float(y[2, 2, 2]) == 1.0 and float(y[0, 0, 0]) == 14.0 and float(y[2, 0, 0]) == 5.0
    x = torch.zeros(1, 3, 3, 3, 1, dtype=torch.float64)
    x[0, 1, 1, 1, 0] = 1.0                           # the centre voxel reaches only itself
    y = MR.conv_same(x, w, zero, 2)[0, ..., 0]
    assert float(y[1, 1, 1]) == 14.0 and float(y.abs().sum()) == 14.0
    # dilation 1 on the same input: the plain 3^3 window, flipped
    y1 = MR.conv_same(x, w, zero, 1)[0, ..., 0]
    assert torch.equal(y1, w[..., 0, 0].flip(0, 1, 2))


def test_bn_is_headtrain_refs_on_a_shared_tensor():
    """The forward's BN statistics, output and (through autograd) backward on
    z_conv4 equal tests/headtrain_ref.py's bn_train / bn_train_bwd closed forms."""
    c = MR.to(MR.case("tiny"))
    q = {k: v.clone().requires_grad_(True) for k, v in c["p"].items()}
    out, aux = MR.forward(q, c["pooled"])
    z, act = aux["z_conv4"], aux["act_bn4"]
    z.retain_grad()
    act.retain_grad()
    MR.HL.mask_loss(c["tmask"], c["ids"], out).backward()
    ch = z.shape[-1]
    gamma, beta = q["mrcnn_mask_bn4/gamma:0"].detach(), q["mrcnn_mask_bn4/beta:0"].detach()
    y, mean, var = HT.bn_train(z.detach().reshape(-1, ch), gamma, beta)
    assert torch.equal(y.reshape(act.shape), act.detach())
    assert torch.equal(mean, aux["mean_bn4"].detach()) and torch.equal(var, aux["var_bn4"].detach())
    dz, dgamma, dbeta = HT.bn_train_bwd(act.grad.reshape(-1, ch), y, z.detach().reshape(-1, ch), gamma, mean, var)
    scale = float(z.grad.abs().max())
    assert float((dz.reshape(z.shape) - z.grad).abs().max()) < 1e-12 * max(scale, 1.0)
    assert float((dgamma - q["mrcnn_mask_bn4/gamma:0"].grad).abs().max()) < 1e-12
    assert float((dbeta - q["mrcnn_mask_bn4/beta:0"].grad).abs().max()) < 1e-12


def test_frozen_forward_on_the_batch_statistics_equals_the_training_forward():
    c = MR.to(MR.case("c5"))
    out, aux = MR.forward(c["p"], c["pooled"])
    p = dict(c["p"])
    for i in ("1", "2", "3", "3b", "4"):
        p[f"mrcnn_mask_bn{i}/moving_mean:0"] = aux[f"mean_bn{i}"]
        p[f"mrcnn_mask_bn{i}/moving_variance:0"] = aux[f"var_bn{i}"]
    frozen, _ = MR.forward(p, c["pooled"], training=False)
    assert float((frozen - out).abs().max()) < 1e-13


def test_relu_masks_reproduce_the_own_branches_and_override_them():
    c = MR.to(MR.case("tiny"))
    out, aux = MR.forward(c["p"], c["pooled"])
    masks = MR.masks_of(aux)
    again, _ = MR.forward(c["p"], c["pooled"], relu_masks=masks)
    assert torch.equal(out, again)
    flipped = dict(masks, bn2=~masks["bn2"])
    other, _ = MR.forward(c["p"], c["pooled"], relu_masks=flipped)
    assert not torch.equal(out, other)
    assert MR.branch_disagreement(masks, aux) == (0.0, 0.0)
    frac, margin = MR.branch_disagreement(flipped, aux)
    assert frac == 1.0 and margin > 1.0


@pytest.mark.parametrize("name", list(MR.CASES))
def test_float32_restatement_meets_the_branch_agreement_bounds(name):
    """What tests/test_gpu_mask_head_train.py asserts of the GPU's sign patterns,
    on the float32 CPU evaluation of the chosen seeds: they differ from
    float64's own only where the float64 pre-activation is within 1e-4 rms of 0,
    and on at most 0.1 % of any layer.  Every case has a positive ROI with a
    non-empty target and an all-zero ROI."""
    c32 = MR.to(MR.case(name), torch.float32)
    _, aux32 = MR.forward(c32["p"], c32["pooled"])
    c = MR.to(MR.case(name))
    _, aux = MR.forward(c["p"], c["pooled"])
    frac, margin = MR.branch_disagreement(MR.masks_of(aux32), aux)
    assert margin <= 1e-4 and frac <= 1e-3, (frac, margin)
    pos = c["ids"] > 0
    assert int(pos.sum()) >= 1 and bool((c["tmask"][pos].flatten(1).sum(1) > 0).all())
    assert float(c["pooled"][-1, -1].abs().max()) == 0.0


def test_param_names_are_the_heads_registration_order():
    from m3d.heads import MaskHead
    from m3d.params import ParamStore
    head = MaskHead(ParamStore(), 2, 32, 32)
    assert tuple(p.name for p in head.params()) == MR.PARAM_NAMES
    assert all(bn.momentum == MR.MOMENTUM for _, bn in head.convs.values())
