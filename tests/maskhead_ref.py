"""Torch restatement of the mask head's training semantics
(build_fpn_mask_graph(train_bn=True), core/models.py:1190-1238), evaluable in
float32 and float64 (the dtype of the inputs is used throughout):

  conv_same       Conv3D(ch, 3^3, 'same', dilation d) as one matmul per tap on
                  the zero-padded volume: y[o] = b + sum_t x[o + (t - 1) d] w[t]
  deconv_k2s2     Conv3DTranspose(ch, 2^3, strides 2), Keras kernel
                  [2,2,2,Cout,Cin]: y[2i + t, o] = b[o] + sum_c x[i, c] w[t, o, c]
  forward         conv + bias -> training-mode BN over all B*N*p^3 rows
                  (tests/headtrain_ref.bn_train) -> ReLU for conv1..3,
                  x = res + relu(bn(conv3b_dil2(res))), conv4, deconv + ReLU, the
                  sigmoid 1^3 conv; ``relu_masks`` replaces each ReLU's sign
                  pattern by a given one (name -> bool tensor: bn1, bn2, bn3,
                  bn3b, bn4, deconv), so the float64 evaluation can take the
                  branches a float32 forward took
  loss_and_grads  forward -> mrcnn_mask_loss (tests/headloss_ref.py) -> autograd:
                  the 24 parameter gradients, d_pooled, and dz of the five convs
                  (the scale of their bias gradients' cancellation)
  SGDSteps        SGD steps on fixed inputs: float64 gradients, the float32
                  Keras update of oracle/optim_ref.py

  case / to      the four test cases (parameters, inputs, targets) shared by the CPU
                  and GPU tests and scripts/measure_maskhead_f32.py

tests/test_maskhead_ref.py pins this file (finite differences, hand-computed
index maps, the shared BN).  CPU float64 checks the kernels
(tests/test_gpu_mask_head_train.py); float32 on the CPU sizes their tolerances.
"""
import functools
import math

import torch

import headloss_ref as HL
import headtrain_ref as HT

MOMENTUM = 0.99                 # BatchNorm() of mrcnn_mask_bn*: the Keras default
CONVS = ("conv1", "conv2", "conv3", "conv3b", "conv4")
ACTS = ("bn1", "bn2", "bn3", "bn3b", "bn4", "deconv")
PARAM_NAMES = tuple(n for c in CONVS for n in (f"mrcnn_mask_{c}/kernel:0", f"mrcnn_mask_{c}/bias:0",
                                               f"mrcnn_mask_bn{c[4:]}/gamma:0", f"mrcnn_mask_bn{c[4:]}/beta:0")) + \
    ("mrcnn_mask_deconv/kernel:0", "mrcnn_mask_deconv/bias:0", "mrcnn_mask/kernel:0", "mrcnn_mask/bias:0")
CONV_BIASES = tuple(f"mrcnn_mask_{c}/bias:0" for c in CONVS)
DILATION = {"conv3b": 2}


def conv_same(x, w, b, d=1):
    """x [M,H,W,D,Cin], w [3,3,3,Cin,Cout]: 'same' at stride 1, dilation d (pad d)."""
    M, H, W, D, _ = x.shape
    xp = torch.nn.functional.pad(x, (0, 0, d, d, d, d, d, d))
    y = None
    for a in range(3):
        for bb in range(3):
            for c in range(3):
                t = xp[:, a * d:a * d + H, bb * d:bb * d + W, c * d:c * d + D] @ w[a, bb, c]
                y = t if y is None else y + t
    return y + b


def deconv_k2s2(x, w, b):
    """x [M,H,W,D,Cin], w [2,2,2,Cout,Cin] -> [M,2H,2W,2D,Cout] (no overlap at stride 2)."""
    M, H, W, D, _ = x.shape
    co = w.shape[3]
    parts = torch.stack([torch.stack([torch.stack([x @ w[a, bb, c].T for c in range(2)], 4)
                                      for bb in range(2)], 3) for a in range(2)], 2)
    # parts [M, H, a, W, b, D, c, Cout]
    return parts.reshape(M, 2 * H, 2 * W, 2 * D, co) + b


def _relu(pre, name, relu_masks):
    if relu_masks is None:
        return torch.relu(pre)
    return pre * relu_masks[name].to(pre.dtype)


def forward(p, pooled, training=True, relu_masks=None):
    """p: dict Keras name -> tensor (the 24 parameters; the ten moving statistics
    too when training is False).  pooled [B,N,p,p,p,Cin].  Returns (mrcnn_mask
    [B,N,2p,2p,2p,C], aux) with aux: z_<conv> (conv + bias), pre_<act> (the value
    each ReLU sees), act_<act> (after it), mean_/var_<bn> in training mode."""
    B, N, ph, pw, pd, cin = pooled.shape
    x = pooled.reshape(B * N, ph, pw, pd, cin)
    aux = {}

    def unit(x, conv):
        i = conv[4:]
        z = conv_same(x, p[f"mrcnn_mask_{conv}/kernel:0"], p[f"mrcnn_mask_{conv}/bias:0"], DILATION.get(conv, 1))
        ch = z.shape[-1]
        g, b = p[f"mrcnn_mask_bn{i}/gamma:0"], p[f"mrcnn_mask_bn{i}/beta:0"]
        if training:
            pre, mean, var = HT.bn_train(z.reshape(-1, ch), g, b, relu=False)
            aux[f"mean_bn{i}"], aux[f"var_bn{i}"] = mean, var
        else:
            pre = HT.bn_frozen(z.reshape(-1, ch), g, b, p[f"mrcnn_mask_bn{i}/moving_mean:0"],
                               p[f"mrcnn_mask_bn{i}/moving_variance:0"])
        pre = pre.reshape(z.shape)
        y = _relu(pre, f"bn{i}", relu_masks)
        aux[f"z_{conv}"], aux[f"pre_bn{i}"], aux[f"act_bn{i}"] = z, pre, y
        return y
    x = unit(x, "conv1")
    x = unit(x, "conv2")
    res = unit(x, "conv3")
    x = res + unit(res, "conv3b")
    x = unit(x, "conv4")
    pre = deconv_k2s2(x, p["mrcnn_mask_deconv/kernel:0"], p["mrcnn_mask_deconv/bias:0"])
    up = _relu(pre, "deconv", relu_masks)
    aux["pre_deconv"], aux["act_deconv"] = pre, up
    ch, C = p["mrcnn_mask/kernel:0"].shape[-2:]
    out = torch.sigmoid(up @ p["mrcnn_mask/kernel:0"].reshape(ch, C) + p["mrcnn_mask/bias:0"])
    return out.reshape(B, N, 2 * ph, 2 * pw, 2 * pd, C), aux


def loss_and_grads(p, pooled, target_class_ids, target_mask, relu_masks=None, pooled_grad=True):
    """One training-mode forward + mrcnn_mask_loss + autograd: returns (loss,
    grads {name: tensor}, d_pooled, mrcnn_mask, aux); aux["z_<conv>"].grad holds dz."""
    q = {k: v.detach().clone().requires_grad_(k in PARAM_NAMES) for k, v in p.items()}
    x = pooled.detach().clone().requires_grad_(pooled_grad)
    out, aux = forward(q, x, True, relu_masks)
    for c in CONVS:
        aux[f"z_{c}"].retain_grad()
    loss = HL.mask_loss(target_mask, target_class_ids, out)
    loss.backward()
    grads = {k: (q[k].grad if q[k].grad is not None else torch.zeros_like(q[k])) for k in PARAM_NAMES}
    return loss.detach(), grads, x.grad, out.detach(), aux


def masks_of(aux):
    """The sign pattern each ReLU took: name -> bool tensor."""
    return {k: aux[f"pre_{k}"].detach() > 0 for k in ACTS}


def moving_after(moving, aux, rows):
    """{bn: (mean, var)} after one training forward (momentum 0.99)."""
    return {k: HT.moving_update(mm, mv, aux[f"mean_{k}"].detach(), aux[f"var_{k}"].detach(), rows, MOMENTUM)
            for k, (mm, mv) in moving.items()}


class SGDSteps:
    """SGD steps on fixed inputs: gradients in the dtype of ``pooled``, the Keras
    update in float32 by oracle/optim_ref.step.  ``step(relu_masks)`` runs one
    step (optionally on a given sign pattern, e.g. the one the float32 forward of
    the same step took) and returns (loss before the update, aux); ``cur`` holds
    the float32 parameters {name: numpy}."""

    def __init__(self, p, pooled, target_class_ids, target_mask, lr, momentum):
        self.cur = {k: v.detach().float().numpy().copy() for k, v in p.items()}
        self.args = (pooled, target_class_ids, target_mask)
        self.lr, self.momentum, self.it = lr, momentum, 0
        self.slots = {k: {} for k in PARAM_NAMES}

    def step(self, relu_masks=None):
        from oracle import optim_ref
        q = {k: torch.from_numpy(v).to(self.args[0].dtype) for k, v in self.cur.items()}
        loss, grads, _, _, aux = loss_and_grads(q, *self.args, relu_masks, pooled_grad=False)
        for k in PARAM_NAMES:
            self.cur[k] = optim_ref.step("SGD", self.cur[k], grads[k].float().numpy(), self.slots[k], self.it, self.lr,
                                         momentum=self.momentum)
        self.it += 1
        return float(loss), aux


# (p, Cin, ch, C, B, N, seed): tests/test_gpu_mask_head_train.py says what each exercises
CASES = {"tiny": (3, 32, 32, 2, 2, 3, 0), "wino": (6, 64, 64, 2, 1, 13, 1), "c5": (4, 32, 32, 5, 1, 4, 2),
         "real": (14, 64, 64, 2, 1, 2, 3)}


@functools.lru_cache(maxsize=None)
def case(name):
    """float32 host parameters / inputs / targets / moving statistics of one case (torch, CPU).
    The last ROI is all zero (a zero-padded ROI counts in the batch statistics)."""
    ps, cin, ch, C, B, N, seed = CASES[name]
    g = torch.Generator().manual_seed(700 + seed)

    def rn(*s, scale=1.0):
        return torch.randn(*s, generator=g) * scale
    p, moving = {}, {}
    c_in = cin
    for conv in CONVS:
        i = conv[4:]
        p[f"mrcnn_mask_{conv}/kernel:0"] = rn(3, 3, 3, c_in, ch, scale=1 / math.sqrt(27 * c_in))
        p[f"mrcnn_mask_{conv}/bias:0"] = rn(ch, scale=0.1)
        p[f"mrcnn_mask_bn{i}/gamma:0"] = rn(ch, scale=0.2) + 1.0
        p[f"mrcnn_mask_bn{i}/beta:0"] = rn(ch, scale=0.3)
        moving[f"bn{i}"] = (rn(ch, scale=0.2), torch.rand(ch, generator=g) + 0.5)
        c_in = ch
    p["mrcnn_mask_deconv/kernel:0"] = rn(2, 2, 2, ch, ch, scale=1 / math.sqrt(ch))
    p["mrcnn_mask_deconv/bias:0"] = rn(ch, scale=0.1)
    p["mrcnn_mask/kernel:0"] = rn(1, 1, 1, ch, C, scale=2 / math.sqrt(ch))
    p["mrcnn_mask/bias:0"] = rn(C, scale=0.1)
    pooled = rn(B, N, ps, ps, ps, cin)
    pooled[-1, -1] = 0.0
    ids = torch.randint(0, C, (B, N), generator=g, dtype=torch.int32)
    ids[:, 0] = 1                           # at least one positive per image
    tmask = (torch.rand(B, N, 2 * ps, 2 * ps, 2 * ps, generator=g) > 0.5).float()
    return dict(p=p, pooled=pooled, ids=ids, tmask=tmask, moving=moving, C=C, ch=ch)


def to(c, dtype=torch.float64):
    f = lambda t: t.to(dtype)                                                   # noqa: E731
    return dict(p={k: f(v) for k, v in c["p"].items()}, pooled=f(c["pooled"]), ids=c["ids"].long(),
                tmask=f(c["tmask"]), moving={k: (f(a), f(b)) for k, (a, b) in c["moving"].items()},
                C=c["C"], ch=c["ch"])


def branch_disagreement(masks, aux64):
    """How a forward's ReLU sign patterns ``masks`` differ from the float64
    evaluation's own (aux64 of a forward WITHOUT relu_masks): per layer, the
    fraction of differing entries, and the largest |float64 pre-activation| / rms
    among them (0 where none differ)."""
    worst_frac = worst_margin = 0.0
    for k in ACTS:
        pre = aux64[f"pre_{k}"].detach()
        diff = masks[k].reshape(pre.shape).cpu() != (pre > 0)
        worst_frac = max(worst_frac, float(diff.double().mean()))
        if bool(diff.any()):
            worst_margin = max(worst_margin, float(pre[diff].abs().max() / pre.pow(2).mean().sqrt()))
    return worst_frac, worst_margin


def rel(got, ref):
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).detach().double()
    return float((got.reshape(ref.shape) - ref).abs().max()) / float(ref.abs().max())


def errors(loss, grads, d_pooled, ref):
    """Errors of one step against ref = dict(loss, grads, d_pooled, aux) (a float64
    loss_and_grads): the loss relative to max(1, |ref|); the 19 non-cancelling
    parameter gradients and d_pooled relative to the reference tensor's largest
    entry; the five conv bias gradients (cancellations to about 0 under batch
    statistics) per column relative to that column's sum |dz|."""
    lr = float(ref["loss"])
    bias = 0.0
    for conv, k in zip(CONVS, CONV_BIASES):
        dz = ref["aux"][f"z_{conv}"].grad
        scale = dz.reshape(-1, dz.shape[-1]).abs().sum(0)
        bias = max(bias, float(((torch.as_tensor(grads[k]).detach().double().cpu() - ref["grads"][k]).abs() / scale).max()))
    return {"loss": abs(float(loss) - lr) / max(1.0, abs(lr)),
            "grad": max(rel(grads[k], ref["grads"][k]) for k in PARAM_NAMES if k not in CONV_BIASES),
            "bias": bias, "d_pooled": rel(d_pooled, ref["d_pooled"])}


def reference_on(name, relu_masks):
    """float64 loss_and_grads of a case on a given sign pattern, as a dict."""
    c = to(case(name))
    loss, grads, d_pooled, out, aux = loss_and_grads(c["p"], c["pooled"], c["ids"], c["tmask"], relu_masks)
    return dict(loss=loss, grads=grads, d_pooled=d_pooled, out=out, aux=aux)
