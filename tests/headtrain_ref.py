"""Torch restatement of the classifier head's training semantics, evaluable in
float32 and float64 (the dtype of the inputs is used throughout):

  bn_train        Keras 2.3.1 BatchNormalization.call(training=True) on the TF
                  backend's non-fused path under TimeDistributed: statistics
                  over all M rows of z [M, C], biased two-pass variance
  moving_update   moving_mean <- moving_mean*mom + mean*(1 - mom);
                  moving_variance <- moving_variance*mom
                                     + var*M/(M - (1 + eps))*(1 - mom)
  bn_train_bwd    the closed-form backward (dbeta, dgamma, dz)
  head_forward    fpn_classifier_graph (core/models.py:1121-1187) as one GEMM
                  per layer, training or inference BN, the clip on the logits
  max_norm        keras.constraints.MaxNorm(max_value, axis=0)
  train_steps     forward -> class + bbox loss (tests/headloss_ref.py) ->
                  autograd -> Keras SGD / Adam with the l2(wd)(w)/size(w) term on
                  kernels and biases -> MaxNorm, repeated on fixed inputs

CPU float64 is the checker of the kernels (tests/test_gpu_bn_train.py,
tests/test_gpu_head_train.py); float32 on the CPU sizes their tolerances.
Gradients of head_forward come from autograd; tests/test_headtrain_ref.py pins
this file (hand-computed BN case, gradcheck, oracle/heads_ref in inference
mode, MaxNorm known answers).
"""
import numpy as np
import torch

import headloss_ref as HL

EPS_BN = 1e-3
K_EPSILON = 1e-7
HEAD_MOMENTUM = 0.9            # BatchNorm(momentum=0.9) of mrcnn_class_bn1 / bn2
MAX_NORM = {"mrcnn_class_logits/kernel:0": 2.0, "mrcnn_bbox_fc/kernel:0": 1.0}
L2_NAMES = ("kernel:0", "bias:0")          # the reference regularises kernels and biases, never gamma/beta


def bn_train(z, gamma, beta, eps=EPS_BN, relu=True):
    """y, mean, var of training-mode BN over the rows of z [M, C]."""
    M = z.shape[0]
    mean = z.sum(0) / M
    var = ((z - mean) ** 2).sum(0) / M
    rstd = 1.0 / torch.sqrt(var + eps)
    y = gamma * ((z - mean) * rstd) + beta
    return (torch.relu(y) if relu else y), mean, var


def moving_update(moving_mean, moving_variance, mean, var, M, momentum, eps=EPS_BN):
    mm = moving_mean * momentum + mean * (1.0 - momentum)
    mv = moving_variance * momentum + var * (M / (M - (1.0 + eps))) * (1.0 - momentum)
    return mm, mv


def bn_train_bwd(dy, y, z, gamma, mean, var, eps=EPS_BN, relu=True):
    """(dz, dgamma, dbeta) in closed form."""
    M = z.shape[0]
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (z - mean) * rstd
    dpre = dy * (y > 0).to(dy.dtype) if relu else dy
    dbeta = dpre.sum(0)
    dgamma = (dpre * xhat).sum(0)
    dz = gamma * rstd * (dpre - dbeta / M - xhat * dgamma / M)
    return dz, dgamma, dbeta


def bn_frozen(z, gamma, beta, mean, var, eps=EPS_BN):
    return (z - mean) * (gamma / torch.sqrt(var + eps)) + beta


def head_forward(p, pooled, num_classes, training=True, eps=EPS_BN):
    """p: dict Keras name -> tensor (the twelve parameters; the four moving
    statistics too when training is False).  pooled [B,N,s,s,s,C].
    Returns (logits [B,N,C] clipped, probs, bbox [B,N,C,6], aux) with aux =
    dict of the pre-clip raw logits, both BN pre-activations (gamma xhat + beta)
    and, in training mode, the batch statistics."""
    B, N = pooled.shape[:2]
    M = B * N
    x = pooled.reshape(M, -1)
    fc = p["mrcnn_class_conv1/bias:0"].shape[0]
    aux = {}
    h = x
    for i, conv in ((1, "mrcnn_class_conv1"), (2, "mrcnn_class_conv2")):
        z = h @ p[f"{conv}/kernel:0"].reshape(-1, fc) + p[f"{conv}/bias:0"]
        g, b = p[f"mrcnn_class_bn{i}/gamma:0"], p[f"mrcnn_class_bn{i}/beta:0"]
        if training:
            pre, mean, var = bn_train(z, g, b, eps, relu=False)
            aux[f"mean{i}"], aux[f"var{i}"] = mean, var
        else:
            pre = bn_frozen(z, g, b, p[f"mrcnn_class_bn{i}/moving_mean:0"],
                            p[f"mrcnn_class_bn{i}/moving_variance:0"], eps)
        aux[f"z{i}"], aux[f"pre{i}"] = z, pre
        h = torch.relu(pre)
    raw = h @ p["mrcnn_class_logits/kernel:0"] + p["mrcnn_class_logits/bias:0"]
    aux["raw_logits"] = raw
    logits = raw.clamp(-10.0, 10.0)
    probs = torch.softmax(logits, -1)
    bbox = h @ p["mrcnn_bbox_fc/kernel:0"] + p["mrcnn_bbox_fc/bias:0"]
    C = num_classes
    return logits.reshape(B, N, C), probs.reshape(B, N, C), bbox.reshape(B, N, C, 6), aux


def max_norm(w, max_value, axis=0):
    norms = torch.sqrt((w * w).sum(axis, keepdim=True))
    desired = norms.clamp(0.0, max_value)
    return w * (desired / (K_EPSILON + norms))


PARAM_NAMES = tuple(f"{layer}/{t}" for layer, ts in (
    ("mrcnn_class_conv1", ("kernel:0", "bias:0")), ("mrcnn_class_bn1", ("gamma:0", "beta:0")),
    ("mrcnn_class_conv2", ("kernel:0", "bias:0")), ("mrcnn_class_bn2", ("gamma:0", "beta:0")),
    ("mrcnn_class_logits", ("kernel:0", "bias:0")), ("mrcnn_bbox_fc", ("kernel:0", "bias:0"))) for t in ts)


def loss_and_grads(p, pooled, target_class_ids, target_bbox, active, num_classes, weights=(1.0, 1.0),
                   pooled_grad=True):
    """One training-mode forward + the class / bbox losses + autograd:
    returns (total, lc, lb, grads {name: tensor}, d_pooled, outputs, aux)."""
    q = {k: v.detach().clone().requires_grad_(k in PARAM_NAMES) for k, v in p.items()}
    x = pooled.detach().clone().requires_grad_(pooled_grad)
    logits, probs, bbox, aux = head_forward(q, x, num_classes, training=True)
    aux["z1"].retain_grad()                 # dz1 / dz2: the scale of the conv bias gradients' cancellation
    aux["z2"].retain_grad()
    lc = HL.class_loss(target_class_ids, logits, active)
    lb = HL.bbox_loss(target_bbox, target_class_ids, bbox)
    total = lc * weights[0] + lb * weights[1]
    total.backward()
    grads = {k: (q[k].grad if q[k].grad is not None else torch.zeros_like(q[k])) for k in PARAM_NAMES}
    return total.detach(), lc.detach(), lb.detach(), grads, x.grad, (logits.detach(), probs.detach(),
                                                                     bbox.detach()), aux


def train_steps(p, moving, pooled, target_class_ids, target_bbox, active, num_classes, steps, optimizer,
                weight_decay=0.0, weights=(1.0, 1.0), momentum_bn=HEAD_MOMENTUM):
    """``steps`` head-only steps on fixed inputs.  optimizer: ("SGD", lr,
    momentum) or ("ADAM", lr, beta_1, beta_2, epsilon) with Keras 2.3.1's update
    formulas; the l2 term weight_decay/size(w) * w is added to the gradient of
    kernels and biases.  Returns (per step [total, class, bbox, the smallest
    |BN pre-activation| / rms of that step], final params, final moving
    statistics {bn1: (mean, var), bn2: ...})."""
    p = {k: v.detach().clone() for k, v in p.items()}
    moving = {k: (a.detach().clone(), b.detach().clone()) for k, (a, b) in moving.items()}
    slots = {k: [torch.zeros_like(p[k]), torch.zeros_like(p[k])] for k in PARAM_NAMES}
    M = pooled.shape[0] * pooled.shape[1]
    traj = []
    for it in range(steps):
        total, lc, lb, grads, _, _, aux = loss_and_grads(p, pooled, target_class_ids, target_bbox, active,
                                                         num_classes, weights, pooled_grad=False)
        rms = [float(aux[f"pre{i}"].detach().pow(2).mean().sqrt()) for i in (1, 2)]
        margin = min(float(aux[f"pre{i}"].detach().abs().min()) / rms[i - 1] for i in (1, 2))
        traj.append((float(total), float(lc), float(lb), margin))
        for i in (1, 2):
            moving[f"bn{i}"] = moving_update(*moving[f"bn{i}"], aux[f"mean{i}"].detach(), aux[f"var{i}"].detach(),
                                             M, momentum_bn)
        for k in PARAM_NAMES:
            g = grads[k]
            if k.endswith(L2_NAMES):
                g = g + (weight_decay / p[k].numel()) * p[k]
            if optimizer[0] == "SGD":
                _, lr, mom = optimizer
                slots[k][0] = mom * slots[k][0] - lr * g
                p[k] = p[k] + slots[k][0]
            else:
                _, lr, b1, b2, eps = optimizer
                t = it + 1
                lr_t = lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
                slots[k][0] = b1 * slots[k][0] + (1.0 - b1) * g
                slots[k][1] = b2 * slots[k][1] + (1.0 - b2) * (g * g)
                p[k] = p[k] - (lr_t * slots[k][0]) / (torch.sqrt(slots[k][1]) + eps)
        for k, mx in MAX_NORM.items():
            p[k] = max_norm(p[k], mx)
    return np.array(traj), p, moving
