"""Mask R-CNN heads, DetectionLayer and the full inference model on libm3d.

Mirrors the reference's inference graph (MaskRCNN.build, MODE "inference",
core/models.py:5473-5760):

  backbone + FPN + RPN -> ProposalLayer(POST_NMS_ROIS_INFERENCE)
  -> PyramidROIAlign(POOL_SIZE) -> fpn_classifier_graph   (1121-1186)
  -> DetectionLayer (refine_detections_graph)            (1415-1575)
  -> PyramidROIAlign(MASK_POOL_SIZE) on the detections -> build_fpn_mask_graph (1190-1234)

Layer names follow the Keras weights (mrcnn_class_conv1, mrcnn_class_bn1, ...,
mrcnn_mask_deconv, mrcnn_mask) so an H5 importer maps 1:1.  Every op is a
libm3d kernel:
  * mrcnn_class_conv1 (a pool^3 'valid' conv = one GEMM with K = pool^3*C):
    split-K batched GEMM + deterministic reduce with the fused BN/ReLU;
  * mrcnn_class_conv2 (1^3): conv kernel with fused bias/BN/ReLU;
  * the two Dense heads: one GEMM over the concatenated kernels, then
    m3d_head_outputs (clip, softmax, bbox reshape);
  * mask convs: conv kernel (Winograd for 3^3 'same'), the dilated conv3b with
    its post-activation residual Add fused in the epilogue, the 2x2x2 stride-2
    transposed conv as one GEMM with a scattering epilogue, the sigmoid 1^3 conv;
  * DetectionLayer: m3d_refine_detections + 2-D m3d_nms3d + m3d_detections_gather.
Inference runs every BN on moving statistics (TRAIN_BN=False).
MaskRCNN.head_losses scores a checkpoint with the three head losses of the
training graph (m3d.head_losses).  The classifier head also trains:
ClassifierHead(pooled, training=True) runs its two BNs on batch statistics
(m3d_bn_train_fwd, Keras training-mode semantics, moving statistics updated)
and its backward (_ClassifierHeadTrain) writes the head's twelve parameter
gradients into the ParamStore and returns the gradient of the pooled features;
MaskRCNN.train_classifier_head is one head-only optimizer step.  The mask head
trains the same way (build_fpn_mask_graph(train_bn=True), core/models.py:
1190-1238): MaskHead(pooled, training=True) runs its five BNs on batch
statistics over all B*N*p^3 rows (momentum 0.99) and composes the backward from
  * the conv units' own autograd (conv + bias with the tree's direct / Winograd
    forward, data-gradient and weight-gradient routing) and _BNTrainAct;
  * _MaskResDil: the dilated conv3b branch, whose data gradient accumulates
    into the incoming gradient (d_res = d_x + dgrad_dil(dz), accumulate = 1);
  * _MaskTail: m3d_mask_out_bwd (sigmoid conv backward + the deconv's ReLU mask
    + three of the parameter gradients in one pass) and the transposed conv's
    two gradients;
24 parameter gradients added into the ParamStore, d_pooled returned; the weight
gradients run on m3d.nn's weight-gradient stream and the backward pass ends
with its join.  MaskRCNN.train_heads is one optimizer step on both heads (or
either) against the LOSS_WEIGHTS-weighted head losses, the trunk frozen.  The
join of d_pooled / d_mask_pooled into PyramidROIAlign's backward and the trunk
is not built.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib, ops
from ._lib import check, ptr, stream
from .anchors import model_anchors
from .backbone import FPN, ResNet3D, RPNHead
from .layers import ProposalLayer, PyramidROIAlign
from .nn import conv_bn_act, conv_geom
from .params import BNLayer, ConvLayer, ParamStore


def _L():
    return _lib.load()


def _bn_affine(bn):
    aff = torch.empty((3, bn.c), device=bn.gamma.data.device, dtype=torch.float32)
    check(_L().m3d_bn_affine(ptr(bn.gamma.data), ptr(bn.beta.data), ptr(bn.moving_mean),
                             ptr(bn.moving_variance), float(bn.eps), bn.c, ptr(aff[1]), ptr(aff[2]),
                             ptr(aff[0]), stream()), "bn_affine")
    return aff[1], aff[2]


class DenseLayer:
    """KL.Dense kernel [in, out] + bias (Keras names <name>/kernel:0, bias:0)."""

    def __init__(self, store, name, cin, cout, kernel_init="glorot_uniform", bias_init="zeros"):
        self.name, self.cin, self.cout = name, cin, cout
        self.kernel = store.add(f"{name}/kernel:0", (cin, cout), kernel_init, True)
        self.bias = store.add(f"{name}/bias:0", (cout,), bias_init, True)


def _params_chunk_range(store, ps, what):
    """(first, end) chunk of the consecutively registered parameters ``ps``."""
    from .params import CHUNK
    i0 = store.params.index(ps[0])
    if store.params[i0:i0 + len(ps)] != ps:
        raise RuntimeError(f"{what} parameters are not consecutive in the store")
    last = ps[-1]
    return ps[0].offset // CHUNK, (last.offset + -(-last.numel // CHUNK) * CHUNK) // CHUNK


class ClassifierHead:
    """fpn_classifier_graph(y, pool_size, num_classes, fc_layers_size, train_bn=False)."""

    SPLITK_TARGET_BLOCKS = 512

    def __init__(self, store, pool_size, num_classes, fc_layers_size, channels=256):
        p, fc = pool_size, fc_layers_size
        self.pool, self.C, self.fc, self.cin = p, num_classes, fc, channels
        self.store = store
        self.conv1 = ConvLayer(store, "mrcnn_class_conv1", (p, p, p), channels, fc)
        self.bn1 = BNLayer(store, "mrcnn_class_bn1", fc, momentum=0.9)      # BatchNorm(momentum=0.9)
        self.conv2 = ConvLayer(store, "mrcnn_class_conv2", (1, 1, 1), fc, fc)
        self.bn2 = BNLayer(store, "mrcnn_class_bn2", fc, momentum=0.9)
        fg = 0.15
        # the reference's prior bias is (bg, fg) for its two classes; with more classes every
        # foreground class takes the fg value (the reference graph cannot be built there)
        self.logits = DenseLayer(store, "mrcnn_class_logits", fc, num_classes, ("normal", 0.01),
                                 ("const", [-math.log((1 - fg) / fg)] +
                                  [math.log(fg / (1 - fg))] * (num_classes - 1)))
        self.bbox = DenseLayer(store, "mrcnn_bbox_fc", fc, num_classes * 6, ("normal", 0.001))
        # kernel_constraint=MaxNorm(max_value) of the two Dense layers (core/models.py:1160, 1175)
        self.max_norm_constraints = {"mrcnn_class_logits/kernel:0": 2.0, "mrcnn_bbox_fc/kernel:0": 1.0}

    def params(self):
        """The head's twelve trainable tensors, in registration order."""
        return [self.conv1.kernel, self.conv1.bias, self.bn1.gamma, self.bn1.beta,
                self.conv2.kernel, self.conv2.bias, self.bn2.gamma, self.bn2.beta,
                self.logits.kernel, self.logits.bias, self.bbox.kernel, self.bbox.bias]

    def chunk_range(self):
        """(first, end) chunk of the head's parameters in the finalized store:
        they are registered consecutively, so KerasOptimizer.step(store,
        chunks=...) on this range is a head-only step."""
        return _params_chunk_range(self.store, self.params(), "classifier head")

    def _conv1(self, x2d, bn=True):
        """[M, K] @ [K, fc] with split-K (K = pool^3 * C is ~88k for 7^3x256).
        bn: apply bn1's moving-statistics affine and the ReLU in the reduce
        (inference); False: conv + bias only (the training mode's z1)."""
        L = _L()
        M, K = x2d.shape
        fc = self.fc
        tiles = -(-M // 128) * -(-fc // 128)
        splits = max(1, min(64, self.SPLITK_TARGET_BLOCKS // max(tiles, 1), K // 1024))
        kc = -(-(-(-K // splits)) // 32) * 32                  # slice width, multiple of 32
        splits = -(-K // kc)
        ws = torch.empty((splits, M, fc), device=x2d.device, dtype=torch.float32)
        w = self.conv1.kernel.data.reshape(K, fc)
        full = K // kc
        if full:
            check(L.m3d_gemm_f32_ex(ptr(x2d), K, kc, ptr(w), kc * fc, ptr(ws), M * fc, full, M, kc, fc,
                                    None, 0, 0, stream()), "class_conv1 gemm")
        if full < splits:
            rem = K - full * kc
            check(L.m3d_gemm_f32_ex(x2d.data_ptr() + 4 * full * kc, K, 0, w[full * kc:].data_ptr(), 0,
                                    ws[full].data_ptr(), 0, 1, M, rem, fc, None, 0, 0, stream()),
                  "class_conv1 gemm tail")
        scale, shift = _bn_affine(self.bn1) if bn else (None, None)
        h = torch.empty((M, fc), device=x2d.device, dtype=torch.float32)
        check(L.m3d_splitk_reduce(ptr(ws), splits, M, fc, ptr(self.conv1.bias.data), ptr(scale), ptr(shift),
                                  1 if bn else 0, ptr(h), stream()), "class_conv1 reduce")
        return h

    def __call__(self, pooled, training=False):
        """training=False: moving-statistics BN (the inference graph).
        training=True: batch-statistics BN over all B*N ROIs (zero-padded ones
        included, as under TimeDistributed), the moving statistics updated once;
        the outputs carry the head's backward (see _ClassifierHeadTrain)."""
        if training:
            return _ClassifierHeadTrain.apply(pooled, self.conv1.kernel.data, self)
        B, N = pooled.shape[:2]
        h = self._conv1(pooled.reshape(B * N, -1).contiguous())
        scale, shift = _bn_affine(self.bn2)
        h2 = torch.empty_like(h)
        _conv1_rows(h, self.conv2.kernel.data, self.conv2.bias.data, h2, "class_conv2", scale, shift, act=1)
        return self._outputs(h2, B, N, 4)[:3]

    def _dense_cat(self, pad):
        """(wcat [fc, nraw], bcat [nraw], nraw): the two Dense layers' kernels and
        biases side by side, the 7 C columns zero-padded to a multiple of ``pad``."""
        C, dev = self.C, self.logits.kernel.data.device
        nraw = -(-7 * C // pad) * pad
        wcat = torch.zeros((self.fc, nraw), device=dev, dtype=torch.float32)
        wcat[:, :C] = self.logits.kernel.data
        wcat[:, C:7 * C] = self.bbox.kernel.data
        bcat = torch.zeros((nraw,), device=dev, dtype=torch.float32)
        bcat[:C] = self.logits.bias.data
        bcat[C:7 * C] = self.bbox.bias.data
        return wcat, bcat, nraw

    def _outputs(self, h, B, N, pad):
        """The concatenated Dense GEMM on h [B*N, fc] and m3d_head_outputs (clip,
        softmax, bbox reshape): (logits, probs, bbox, raw, wcat)."""
        L = _L()
        M, C = B * N, self.C
        wcat, bcat, nraw = self._dense_cat(pad)
        raw = torch.empty((M, nraw), device=h.device, dtype=torch.float32)
        check(L.m3d_gemm_f32_ex(ptr(h), self.fc, 0, ptr(wcat), 0, ptr(raw), 0, 1, M, self.fc, nraw,
                                ptr(bcat), 0, 0, stream()), "class dense")
        logits = torch.empty((B, N, C), device=h.device, dtype=torch.float32)
        probs = torch.empty_like(logits)
        bbox = torch.empty((B, N, C, 6), device=h.device, dtype=torch.float32)
        check(L.m3d_head_outputs(ptr(raw), M, nraw, C, ptr(logits), ptr(probs), ptr(bbox), stream()),
              "head_outputs")
        return logits, probs, bbox, raw, wcat


def bn_train_few_rows_max():
    """M3D_BN_TRAIN_FEW_ROWS_MAX of the loaded library: up to this many rows
    m3d_bn_train_fwd / _bwd run as one launch with a workgroup per 16-channel
    strip; above it they go through per-row-block partial sums."""
    return int(_L().m3d_bn_train_few_rows_max())


def _bn_train_ws(M, C, dev):
    n = int(_L().m3d_bn_train_workspace_bytes(M, C))
    return (torch.empty(n // 4, device=dev, dtype=torch.float32) if n else None), n


def bn_train_fwd(z, bn, relu, y=None, update_moving=True):
    """Keras training-mode BN of z [M, C] on bn's gamma/beta (m3d_bn_train_fwd):
    returns (y, save_mean, save_rstd); bn.moving_mean / moving_variance are
    updated with bn.momentum unless update_moving is False.  y may be z."""
    M, C = z.shape
    y = torch.empty_like(z) if y is None else y
    stats = torch.empty((2, C), device=z.device, dtype=torch.float32)
    ws, wsb = _bn_train_ws(M, C, z.device)
    mm, mv = (bn.moving_mean, bn.moving_variance) if update_moving else (None, None)
    check(_L().m3d_bn_train_fwd(ptr(z), M, C, ptr(bn.gamma.data), ptr(bn.beta.data), float(bn.eps),
                                float(bn.momentum), 1 if relu else 0, ptr(y), ptr(stats[0]), ptr(stats[1]),
                                ptr(mm), ptr(mv), ptr(ws), wsb, stream()), "bn_train_fwd")
    return y, stats[0], stats[1]


def bn_train_bwd(dy, y, z, bn, mean, rstd, relu, dz=None):
    """Backward of bn_train_fwd (m3d_bn_train_bwd): returns dz (dy itself when
    dz is dy) and adds dgamma / dbeta into bn's ParamStore gradient views."""
    M, C = z.shape
    dz = torch.empty_like(dy) if dz is None else dz
    ws, wsb = _bn_train_ws(M, C, z.device)
    check(_L().m3d_bn_train_bwd(ptr(dy), ptr(y), ptr(z), M, C, ptr(bn.gamma.data), ptr(mean), ptr(rstd),
                                1 if relu else 0, ptr(dz), ptr(bn.gamma.grad), ptr(bn.beta.grad), ptr(ws), wsb,
                                stream()), "bn_train_bwd")
    return dz


def _dgrad1(dz, w, cin):
    """dx [M, cin] = dz [M, cout] w^T for a Keras kernel w [cin][cout]: the 1^3
    form of m3d_conv3d_bwd_data over M 'voxels' (cout % 32 == 0, cin % 4 == 0)."""
    M, cout = dz.shape
    dx = torch.empty((M, cin), device=dz.device, dtype=torch.float32)
    check(_L().m3d_conv3d_bwd_data(ptr(dz), ptr(w), 1, 1, 1, M, cin, 1, 1, 1, cout, 1, 1, M, 1, 1, 1, 0, 0, 0,
                                   ptr(dx), 0, stream()), "head dgrad")
    return dx


def _conv1_rows(x, w, b, out, what, scale=None, shift=None, act=0, spill=None):
    """out = act(BN(x w + b)) for x [M rows, cin] and a kernel w [..., cin, cout]:
    the 1^3 form of m3d_conv3d_fwd over M 'voxels' (act 0 none, 1 ReLU, 2
    sigmoid).  out holds the first out.shape[-1] columns; the padded rest, if
    any, goes to ``spill``."""
    cin, cout = w.shape[-2:]
    M, n = x.numel() // cin, out.shape[-1]
    check(_L().m3d_conv3d_fwd(ptr(x), 1, 1, 1, M, cin, ptr(w), 1, 1, 1, cout, 1, 1, M, 1, 1, 1, 0, 0, 0, ptr(b),
                              ptr(scale), ptr(shift), None, 0, act, None, ptr(out), n, ptr(spill), cout - n,
                              n if cout > n else 0, stream()), what)


def _wgrad(a, b, dw):
    """dw [K, N] += a^T b for a [M, K], b [M, N] (m3d_gemm_wgrad_f32; follows
    the process's deterministic mode)."""
    M, K = a.shape
    check(_L().m3d_gemm_wgrad_f32(ptr(a), ptr(b), ptr(dw), 1, M, K, b.shape[1], stream()), "head wgrad")


class _ClassifierHeadTrain(torch.autograd.Function):
    """fpn_classifier_graph(train_bn=True) (core/models.py:1121-1187) with its
    backward.  forward: conv1 (split-K GEMM + bias) -> BN1 batch statistics +
    ReLU -> conv2 (1^3) + bias -> BN2 + ReLU -> the concatenated Dense GEMM ->
    m3d_head_outputs.  backward (from the gradients of logits and bbox, e.g.
    m3d.head_losses.mrcnn_losses): m3d_head_outputs_bwd (clip mask on the
    pre-clip raw), then per layer the weight gradient (m3d_gemm_wgrad_f32), the
    bias gradient (m3d_col_sums_batched), the data gradient (m3d_conv3d_bwd_data,
    1^3 form) and m3d_bn_train_bwd.  The twelve parameter gradients are ADDED
    into their ParamStore views (zero them with store.zero_grad()); the
    returned gradient is d_pooled (only when pooled requires grad).  probs is
    not differentiable here (the losses take the logits).  ``w`` is the conv1
    kernel's ParamStore view: it makes the outputs part of the autograd graph."""

    @staticmethod
    def forward(ctx, pooled, w, head):
        B, N = pooled.shape[:2]
        x = pooled.detach().reshape(B * N, -1).contiguous()
        z1 = head._conv1(x, bn=False)
        y1, mean1, rstd1 = bn_train_fwd(z1, head.bn1, True)
        z2 = torch.empty_like(z1)
        _conv1_rows(y1, head.conv2.kernel.data, head.conv2.bias.data, z2, "class_conv2")
        y2, mean2, rstd2 = bn_train_fwd(z2, head.bn2, True)
        # raw columns padded to a multiple of 32: the data gradient g_raw Wcat^T runs
        # on m3d_conv3d_bwd_data, whose reduction (here nraw) is a multiple of 32
        logits, probs, bbox, raw, wcat = head._outputs(y2, B, N, 32)
        ctx.head, ctx.shape = head, tuple(pooled.shape)
        ctx.save_for_backward(x, z1, y1, mean1, rstd1, z2, y2, mean2, rstd2, raw, wcat)
        ctx.mark_non_differentiable(probs)
        return logits, probs, bbox

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_logits, _g_probs, g_bbox):
        from . import nn as mnn
        L = _L()
        head = ctx.head
        x, z1, y1, mean1, rstd1, z2, y2, mean2, rstd2, raw, wcat = ctx.saved_tensors
        M, nraw = raw.shape
        fc, C, dev = head.fc, head.C, raw.device
        # the weight-gradient GEMMs below run on this stream and, in deterministic mode, through the
        # scratch the side stream's weight gradients use (the mask head's, in a joint backward): wait
        # for those first (nothing to wait for when the classifier trains alone)
        mnn.join_wgrad(dev)
        g_logits = torch.zeros((M, C), device=dev) if g_logits is None else g_logits.contiguous().float()
        g_bbox = torch.zeros((M, C, 6), device=dev) if g_bbox is None else g_bbox.contiguous().float()
        g_raw = torch.empty_like(raw)
        check(L.m3d_head_outputs_bwd(ptr(raw), ptr(g_logits), ptr(g_bbox), M, nraw, C, ptr(g_raw), stream()),
              "head_outputs_bwd")
        # the two Dense layers: kernels and biases through the concatenated layout
        dwcat = torch.zeros_like(wcat)
        dbcat = torch.zeros((nraw,), device=dev, dtype=torch.float32)
        _wgrad(y2, g_raw, dwcat)
        dy2 = _dgrad1(g_raw, wcat, fc)
        dz2 = bn_train_bwd(dy2, y2, z2, head.bn2, mean2, rstd2, True, dz=dy2)
        _wgrad(y1, dz2, head.conv2.kernel.grad.reshape(fc, fc))
        dy1 = _dgrad1(dz2, head.conv2.kernel.data, fc)
        dz1 = bn_train_bwd(dy1, y1, z1, head.bn1, mean1, rstd1, True, dz=dy1)
        _wgrad(x, dz1, head.conv1.kernel.grad.reshape(-1, fc))
        # the bias gradients are the column sums of dz, as TF computes them (about 0
        # under batch statistics for the two convs)
        sums = mnn.BiasSums()
        sums.add(g_raw, M, nraw, dbcat)
        sums.add(dz2, M, fc, head.conv2.bias.grad)
        sums.add(dz1, M, fc, head.conv1.bias.grad)
        sums.flush()
        head.logits.kernel.grad += dwcat[:, :C]
        head.bbox.kernel.grad += dwcat[:, C:7 * C]
        head.logits.bias.grad += dbcat[:C]
        head.bbox.bias.grad += dbcat[C:7 * C]
        d_pooled = None
        if ctx.needs_input_grad[0]:
            d_pooled = _dgrad1(dz1, head.conv1.kernel.data, x.shape[1]).reshape(ctx.shape)
        return d_pooled, None, None


def _on_wgrad_stream(dev, tensors, launch):
    """Run ``launch`` (weight-gradient launches) where the conv units run theirs:
    on m3d.nn's side stream after a fork from the compute stream (one stream at
    a time owns the deterministic-mode scratch), in line when that is off."""
    from . import nn as mnn
    side = mnn._wgrad_stream(dev)
    if side is None:
        launch()
        return
    for t in tensors:
        t.record_stream(side)
    with torch.cuda.stream(side):
        launch()


def _join_after_backward(dev):
    """Queue m3d.nn.join_wgrad for the end of the running backward pass: the
    compute stream then waits for the side stream's weight gradients before
    anything enqueued after backward() reads them."""
    from . import nn as mnn
    torch.autograd.Variable._execution_engine.queue_callback(lambda: mnn.join_wgrad(dev))


class _BNTrainAct(torch.autograd.Function):
    """y = relu(BN(z)) on batch statistics over all rows of z [..., C]
    (BatchNorm()(x, training=True) + Activation('relu'), core/models.py:1202-1203;
    m3d_bn_train_fwd / _bwd, the moving statistics updated once per forward).
    The backward adds dgamma / dbeta into bn's ParamStore views and returns dz.
    ``gamma`` is bn's ParamStore view: it keeps the output in the autograd graph."""

    @staticmethod
    def forward(ctx, z, gamma, bn):
        C = z.shape[-1]
        z = z.contiguous()
        z2 = z.view(-1, C)
        y = torch.empty_like(z)
        _, mean, rstd = bn_train_fwd(z2, bn, True, y=y.view(-1, C))
        ctx.bn = bn
        ctx.save_for_backward(z, y, mean, rstd)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        z, y, mean, rstd = ctx.saved_tensors
        C = z.shape[-1]
        dy = dy.contiguous()
        dz = bn_train_bwd(dy.view(-1, C), y.view(-1, C), z.view(-1, C), ctx.bn, mean, rstd, True)
        return dz.view(z.shape), None, None


class _MaskResDil(torch.autograd.Function):
    """x = res + relu(BN_batch(conv3b_dilated(res) + b)): mrcnn_mask_conv3b /
    bn3b / res3 in training mode (core/models.py:1215-1222).  Returns (x, the
    post-ReLU branch).  backward: m3d_bn_train_bwd, the dilated weight gradient
    (m3d_conv3d_bwd_weight_dil, weight-gradient stream), the bias column sums,
    and d_res = d_x + dgrad_dil(dz) by m3d_conv3d_bwd_data_dil with
    accumulate = 1 into the incoming gradient's own buffer when that buffer is
    a whole tensor (it is conv4's data gradient, which nothing else reads)."""

    DIL = 2

    @staticmethod
    def forward(ctx, res, w, head):
        L = _L()
        layer, bn = head.convs["conv3b"]
        res = res.contiguous()
        M, ph, pw, pd, ch = res.shape
        d = _MaskResDil.DIL
        z = torch.empty_like(res)
        check(L.m3d_conv3d_fwd_dil(ptr(res), M, ph, pw, pd, ch, ptr(layer.kernel.data), 3, 3, 3, ch, ph, pw, pd,
                                   1, 1, 1, d, d, d, d, d, d, ptr(layer.bias.data), None, None, None, 0, 0, None,
                                   ptr(z), ch, None, 0, 0, stream()), "mask_conv3b")
        y = torch.empty_like(z)
        _, mean, rstd = bn_train_fwd(z.view(-1, ch), bn, True, y=y.view(-1, ch))
        x = torch.empty_like(res)
        check(L.m3d_add_f32(ptr(res), ptr(y), ptr(x), res.numel(), stream()), "mask_res3")
        ctx.head = head
        ctx.save_for_backward(res, z, y, mean, rstd)
        ctx.mark_non_differentiable(y)
        return x, y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dx, _dy):
        from . import nn as mnn
        L = _L()
        res, z, y, mean, rstd = ctx.saved_tensors
        layer, bn = ctx.head.convs["conv3b"]
        M, ph, pw, pd, ch = res.shape
        d = _MaskResDil.DIL
        rows = M * ph * pw * pd
        whole = dx.is_contiguous() and dx._base is None and dx.storage_offset() == 0
        dx = dx.contiguous()
        dz = bn_train_bwd(dx.view(rows, ch), y.view(rows, ch), z.view(rows, ch), bn, mean, rstd, True)
        mnn.bias_grad(dz, rows, ch, layer.bias.grad)
        d_res = None
        if ctx.needs_input_grad[0]:
            d_res = dx if whole else dx.clone()
            check(L.m3d_conv3d_bwd_data_dil(ptr(dz), ptr(layer.kernel.data), M, ph, pw, pd, ch, 3, 3, 3, ch, ph, pw,
                                            pd, 1, 1, 1, d, d, d, d, d, d, ptr(d_res), 1, stream()),
                  "mask_conv3b dgrad")
        _on_wgrad_stream(res.device, (res, dz), lambda: check(
            L.m3d_conv3d_bwd_weight_dil(ptr(res), ptr(dz), M, ph, pw, pd, ch, 3, 3, 3, ch, ph, pw, pd, 1, 1, 1,
                                        d, d, d, d, d, d, ptr(layer.kernel.grad), stream()), "mask_conv3b wgrad"))
        return d_res, None, None


class _MaskTail(torch.autograd.Function):
    """mrcnn_mask_deconv (2^3 stride-2 transposed conv + ReLU) and mrcnn_mask
    (1^3 conv + sigmoid), core/models.py:1229-1237.  Returns (mrcnn_mask
    [M,2p,2p,2p,C], the deconv's post-ReLU output).  backward, from the gradient
    of the sigmoid output: m3d_mask_out_bwd (one pass: the sigmoid and ReLU
    masks, g_up, and the mrcnn_mask kernel / bias and deconv bias gradients
    added into their ParamStore views), then m3d_deconv3d_k2s2_bwd_weight
    (weight-gradient stream) and m3d_deconv3d_k2s2_bwd_data."""

    @staticmethod
    def forward(ctx, x, w, head):
        x = x.contiguous()
        up, out = head._tail(x)
        ctx.head = head
        ctx.save_for_backward(x, up, out)
        ctx.mark_non_differentiable(up)
        return out, up

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out, _g_up):
        L = _L()
        head = ctx.head
        x, up, out = ctx.saved_tensors
        M, ph, pw, pd, ch = x.shape
        C = head.C
        V = up.numel() // ch
        _join_after_backward(x.device)
        g_out = g_out.contiguous().float()
        g_up = torch.empty_like(up)
        wsb = int(L.m3d_mask_out_bwd_workspace_bytes(V, ch, C))
        ws = torch.empty(max(wsb // 4, 1), device=x.device, dtype=torch.float32)
        check(L.m3d_mask_out_bwd(ptr(g_out), ptr(out), ptr(up), ptr(head.mask.kernel.data), V, ch, C, ptr(g_up),
                                 ptr(head.mask.kernel.grad), ptr(head.mask.bias.grad), ptr(head.deconv_b.grad),
                                 ptr(ws), wsb, stream()), "mask_out_bwd")
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            check(L.m3d_deconv3d_k2s2_bwd_data(ptr(g_up), ptr(head.deconv.data), M, ph, pw, pd, ch, ch, ptr(dx),
                                               stream()), "mask_deconv dgrad")
        _on_wgrad_stream(x.device, (x, g_up), lambda: check(
            L.m3d_deconv3d_k2s2_bwd_weight(ptr(x), ptr(g_up), M, ph, pw, pd, ch, ch, ptr(head.deconv.grad),
                                           stream()), "mask_deconv wgrad"))
        return dx, None, None


class MaskHead:
    """build_fpn_mask_graph(y, num_classes, conv_channel, train_bn)."""

    ACTIVATIONS = ("bn1", "bn2", "bn3", "bn3b", "bn4", "deconv")

    def __init__(self, store, num_classes, conv_channel, channels=256):
        ch = conv_channel
        self.C, self.ch = num_classes, ch
        self.store = store
        self.convs = {}
        cin = channels
        for name in ("conv1", "conv2", "conv3", "conv3b", "conv4"):
            self.convs[name] = (ConvLayer(store, f"mrcnn_mask_{name}", (3, 3, 3), cin, ch),
                                BNLayer(store, f"mrcnn_mask_bn{name[4:]}", ch))
            cin = ch
        self.deconv = store.add("mrcnn_mask_deconv/kernel:0", (2, 2, 2, ch, ch), "glorot_uniform", True)
        self.deconv_b = store.add("mrcnn_mask_deconv/bias:0", (ch,), "zeros", True)
        self.mask = ConvLayer(store, "mrcnn_mask", (1, 1, 1), ch, num_classes)

    def _same(self, x, name, **kw):
        layer, bn = self.convs[name]
        geo = conv_geom(tuple(x.shape[1:4]), (3, 3, 3), (1, 1, 1), "same")
        return conv_bn_act(x, layer, geo, True, bn=bn, need_dx=False, **kw)

    def params(self):
        """The head's 24 trainable tensors, in registration order: five convs x
        (kernel, bias, gamma, beta), the deconv kernel and bias, the mrcnn_mask
        kernel and bias."""
        ps = []
        for name in ("conv1", "conv2", "conv3", "conv3b", "conv4"):
            layer, bn = self.convs[name]
            ps += [layer.kernel, layer.bias, bn.gamma, bn.beta]
        return ps + [self.deconv, self.deconv_b, self.mask.kernel, self.mask.bias]

    def chunk_range(self):
        """(first, end) chunk of the head's parameters in the finalized store
        (as ClassifierHead.chunk_range)."""
        return _params_chunk_range(self.store, self.params(), "mask head")

    def _tail(self, x):
        """(up, out): relu(deconv(x) + b) [M,2p,2p,2p,ch] and the sigmoid 1^3 conv
        of it [M,2p,2p,2p,C], for x [M,p,p,p,ch]."""
        L = _L()
        M, ph, pw, pd, _ = x.shape
        up = torch.empty((M, 2 * ph, 2 * pw, 2 * pd, self.ch), device=x.device, dtype=torch.float32)
        check(L.m3d_deconv3d_k2s2(ptr(x), M, ph, pw, pd, self.ch, ptr(self.deconv.data), self.ch,
                                  ptr(self.deconv_b.data), 1, ptr(up), stream()), "mask_deconv")
        C = self.C
        cp = -(-C // 4) * 4
        w = torch.zeros((self.ch, cp), device=x.device, dtype=torch.float32)
        w[:, :C] = self.mask.kernel.data.reshape(self.ch, C)
        b = torch.zeros((cp,), device=x.device, dtype=torch.float32)
        b[:C] = self.mask.bias.data
        out = torch.empty((M, 2 * ph, 2 * pw, 2 * pd, C), device=x.device, dtype=torch.float32)
        V = M * 8 * ph * pw * pd
        spill = torch.empty((V, max(cp - C, 1)), device=x.device, dtype=torch.float32)
        _conv1_rows(up, w, b, out, "mrcnn_mask", act=2, spill=spill)
        return up, out

    def _train(self, pooled, return_activations):
        B, N, ph, pw, pd, Cin = pooled.shape
        x = pooled.reshape(B * N, ph, pw, pd, Cin)
        geo = conv_geom((ph, pw, pd), (3, 3, 3), (1, 1, 1), "same")
        acts = {}

        def unit(x, name):
            layer, bn = self.convs[name]
            z = conv_bn_act(x, layer, geo, False, bn=None, need_dx=True)      # conv + bias
            y = _BNTrainAct.apply(z, bn.gamma.data, bn)
            acts["bn" + name[4:]] = y.detach()
            return y
        with torch.enable_grad():
            x = unit(x, "conv1")
            x = unit(x, "conv2")
            res = unit(x, "conv3")
            x, y3b = _MaskResDil.apply(res, self.convs["conv3b"][0].kernel.data, self)
            acts["bn3b"] = y3b
            x = unit(x, "conv4")
            out, up = _MaskTail.apply(x, self.deconv.data, self)
        acts["deconv"] = up
        out = out.view(B, N, 2 * ph, 2 * pw, 2 * pd, self.C)
        if return_activations:
            return out, {k: acts[k] for k in self.ACTIVATIONS}
        return out

    def __call__(self, pooled, training=False, return_activations=False):
        """training=False: moving-statistics BN (the inference graph).
        training=True: every BN on batch statistics over all B*N*p^3 rows
        (zero-padded ROIs included, as under TimeDistributed), the moving
        statistics updated once with momentum 0.99 (BatchNorm()'s default);
        the output carries the head's backward, which ADDS the 24 parameter
        gradients into their ParamStore views and yields d_pooled when pooled
        requires grad.  return_activations (training mode): also a dict of the
        six post-ReLU tensors bn1, bn2, bn3, bn3b, bn4 [B*N,p,p,p,ch] and deconv
        [B*N,2p,2p,2p,ch]."""
        if training:
            return self._train(pooled, return_activations)
        if return_activations:
            raise ValueError("MaskHead: return_activations needs training=True")
        B, N, ph, pw, pd, Cin = pooled.shape
        L = _L()
        x = pooled.reshape(B * N, ph, pw, pd, Cin).contiguous()
        M = B * N
        x = self._same(x, "conv1")
        x = self._same(x, "conv2")
        res = self._same(x, "conv3")
        # x = res + relu(bn(conv3b_dilated(res)))   (mrcnn_mask_res3, post-activation Add)
        layer, bn = self.convs["conv3b"]
        scale, shift = _bn_affine(bn)
        x = torch.empty_like(res)
        check(L.m3d_conv3d_fwd_dil(ptr(res), M, ph, pw, pd, self.ch, ptr(layer.kernel.data), 3, 3, 3, self.ch,
                                   ph, pw, pd, 1, 1, 1, 2, 2, 2, 2, 2, 2, ptr(layer.bias.data), ptr(scale),
                                   ptr(shift), ptr(res), 3, 1, None, ptr(x), self.ch, None, 0, 0, stream()),
              "mask_conv3b")
        x = self._same(x, "conv4")
        _, out = self._tail(x)
        return out.view(B, N, 2 * ph, 2 * pw, 2 * pd, self.C)


class DetectionLayer:
    """DetectionLayer(bbox_std_dev, detection_min_confidence,
    detection_max_instances, detection_nms_threshold, images_per_gpu)
    ([rois, mrcnn_class, mrcnn_bbox, image_meta]) -> [B, max_inst, 8]."""

    def __init__(self, bbox_std_dev, detection_min_confidence, detection_max_instances,
                 detection_nms_threshold, images_per_gpu, *args, name="mrcnn_detection", **kwargs):
        self.std = [float(v) for v in bbox_std_dev]
        self.min_conf = float(detection_min_confidence)
        self.max_inst = int(detection_max_instances)
        self.nms_thr = float(detection_nms_threshold)
        self.images_per_gpu = int(images_per_gpu)
        self.name = name

    def __call__(self, inputs):
        rois, probs, deltas, meta = inputs
        ops._dev(rois, probs, deltas, meta)
        L = _L()
        B, N = rois.shape[:2]
        C = probs.shape[-1]
        dev = rois.device
        det = torch.empty((B, self.max_inst, 8), device=dev, dtype=torch.float32)
        sd = (_lib.c_f * 6)(*[float(np.float32(v)) for v in self.std])
        with torch.no_grad():
            for b in range(B):
                r, p, d = (t[b].detach().float().contiguous() for t in (rois, probs, deltas))
                m = meta[b].detach().float().contiguous()
                bpx = torch.empty((N, 6), device=dev, dtype=torch.float32)
                b2d = torch.empty((N, 4), device=dev, dtype=torch.float32)
                sc = torch.empty((N,), device=dev, dtype=torch.float32)
                check(L.m3d_refine_detections(ptr(r), ptr(p), ptr(d), N, C, ptr(m), sd, self.min_conf,
                                              ptr(bpx), ptr(b2d), ptr(sc), stream()), "refine_detections")
                keep, num = ops.non_max_suppression_3d_padded(b2d, sc, self.max_inst, self.nms_thr, mode="2d")
                check(L.m3d_detections_gather(ptr(bpx), ptr(sc), ptr(keep), ptr(num), self.max_inst, ptr(m),
                                              det[b].data_ptr(), stream()), "detections_gather")
        return det

    def compute_output_shape(self, input_shape):
        return (None, self.max_inst, 8)


class MaskRCNN:
    """MaskRCNN(mode="inference") of the reference on a flat ParamStore:
    detect(image, image_meta) -> detections [B,max_inst,8], mrcnn_class,
    mrcnn_bbox, mrcnn_mask [B,max_inst,2M,2M,2M,C], rpn_rois."""

    def __init__(self, config, device="cuda", seed=1):
        anchors = model_anchors(config, inplace=False)  # patched copy + row-count check (m3d.anchors)
        _lib.load()
        self.config = c = config
        self.device = torch.device(device)
        self.store = ParamStore()
        self.backbone = ResNet3D(self.store, c.BACKBONE, stage5=True, train_bn=c.TRAIN_BN)
        self.fpn = FPN(self.store, c.TOP_DOWN_PYRAMID_SIZE)
        self.rpn = RPNHead(self.store, c.RPN_ANCHOR_STRIDE, len(c.RPN_ANCHOR_RATIOS), c.TOP_DOWN_PYRAMID_SIZE)
        fc = int(getattr(c, "FPN_CLASSIF_FC_LAYERS_SIZE", 512))
        mask_ch = int(getattr(c, "HEAD_CONV_CHANNEL", 256))
        self.classifier = ClassifierHead(self.store, c.POOL_SIZE, c.NUM_CLASSES, fc, c.TOP_DOWN_PYRAMID_SIZE)
        self.mask_head = MaskHead(self.store, c.NUM_CLASSES, mask_ch, c.TOP_DOWN_PYRAMID_SIZE)
        self.store.finalize(self.device, seed=seed)
        self.anchors = torch.from_numpy(anchors).to(self.device)[None]
        self.proposal_layer = ProposalLayer(
            proposal_count=c.POST_NMS_ROIS_INFERENCE, nms_threshold=c.RPN_NMS_THRESHOLD,
            pre_nms_limit=c.PRE_NMS_LIMIT, images_per_gpu=c.IMAGES_PER_GPU,
            rpn_bbox_std_dev=c.RPN_BBOX_STD_DEV, image_depth=c.IMAGE_DEPTH, name="ROI")
        self.roi_align_classifier = PyramidROIAlign([c.POOL_SIZE] * 3, name="roi_align_classifier")
        self.roi_align_mask = PyramidROIAlign([c.MASK_POOL_SIZE] * 3, name="roi_align_mask")
        self.detection = DetectionLayer(c.BBOX_STD_DEV, float(c.DETECTION_MIN_CONFIDENCE),
                                        int(c.DETECTION_MAX_INSTANCES), float(c.DETECTION_NMS_THRESHOLD),
                                        int(c.IMAGES_PER_GPU), name="mrcnn_detection")
        self.proposal_layer_training = self.detection_targets = None    # built by head_losses()

    def _head_targets(self, image, image_meta, gt_class_ids, gt_boxes, gt_masks, seed):
        """The head-training graph up to the sampled ROIs and their targets
        (core/models.py:5586-5620): trunk, ProposalLayer(POST_NMS_ROIS_TRAINING),
        DetectionTargetLayer.  Returns (rpn_rois, rois, target_gt_boxes,
        target_class_ids, target_bbox, target_mask, mrcnn feature maps)."""
        from .targets import DetectionTargetLayer
        c = self.config
        ops._dev(image, image_meta, gt_class_ids, gt_boxes, gt_masks)
        _, C2, C3, C4, C5 = self.backbone(image)
        fmaps = self.fpn(C2, C3, C4, C5)
        _, rpn_probs, rpn_bbox = self.rpn(fmaps)
        if self.proposal_layer_training is None:
            self.proposal_layer_training = ProposalLayer(
                proposal_count=c.POST_NMS_ROIS_TRAINING, nms_threshold=c.RPN_NMS_THRESHOLD,
                pre_nms_limit=c.PRE_NMS_LIMIT, images_per_gpu=c.IMAGES_PER_GPU,
                rpn_bbox_std_dev=c.RPN_BBOX_STD_DEV, image_depth=c.IMAGE_DEPTH, name="ROI")
            self.detection_targets = DetectionTargetLayer(
                c, c.TRAIN_ROIS_PER_IMAGE, c.ROI_POSITIVE_RATIO, c.BBOX_STD_DEV, c.USE_MINI_MASK, c.MASK_SHAPE,
                c.IMAGES_PER_GPU, positive_iou_threshold=c.RPN_POSITIVE_IOU,
                negative_iou_threshold=c.RPN_NEGATIVE_IOU, name="proposal_targets")
        rpn_rois = self.proposal_layer_training([rpn_probs, rpn_bbox, self.anchors])
        h, w, d = (float(v) for v in image.shape[1:4])
        scale = torch.tensor([h, w, d, h, w, d], device=image.device, dtype=torch.float32)
        gt_norm = gt_boxes.to(torch.float32) / scale
        rois, target_gt_boxes, target_class_ids, target_bbox, target_mask = self.detection_targets(
            [rpn_rois, gt_class_ids, gt_norm, gt_masks], seed=seed)
        mrcnn_maps = fmaps[:4]
        return rpn_rois, rois, target_gt_boxes, target_class_ids, target_bbox, target_mask, mrcnn_maps

    @torch.no_grad()
    def head_losses(self, image, image_meta, gt_class_ids, gt_boxes, gt_masks, seed=None):
        """The three head losses of the reference's head-training graph
        (MaskRCNN.build, MODE "training", core/models.py:5586-5660) for one batch:

          backbone + FPN + RPN -> ProposalLayer(POST_NMS_ROIS_TRAINING)
          -> DetectionTargetLayer(config) on the pixel gt_boxes normalised by
             (H,W,D,H,W,D) (norm_boxes_graph), gt_class_ids [B,G], gt_masks [B,H,W,D,G]
          -> PyramidROIAlign(POOL_SIZE) / (MASK_POOL_SIZE) on the sampled ROIs
          -> classifier head / mask head -> m3d.head_losses.mrcnn_losses
             with active_class_ids = image_meta[:, 16:] and the config's LOSS_WEIGHTS.

        Returns a dict: "loss" (weighted total), "mrcnn_class_loss",
        "mrcnn_bbox_loss", "mrcnn_mask_loss" (device scalars) and the
        intermediates (rpn_rois, rois, target_gt_boxes, target_class_ids,
        target_bbox, target_mask, mrcnn_class_logits, mrcnn_class, mrcnn_bbox,
        mrcnn_mask, active_class_ids).  ``seed`` fixes DetectionTargetLayer's
        sampling order.

        The heads run with moving-statistics BN, as everywhere in this tree.  The
        reference's training graph runs the head BNs on batch statistics
        (train_bn=True, core/models.py:5624,5636), so this is the validation
        score of a checkpoint, not that graph's training-mode value."""
        from .head_losses import active_class_ids_from_meta, mrcnn_losses
        rpn_rois, rois, target_gt_boxes, target_class_ids, target_bbox, target_mask, mrcnn_maps = \
            self._head_targets(image, image_meta, gt_class_ids, gt_boxes, gt_masks, seed)
        pooled = self.roi_align_classifier([rois, image_meta] + mrcnn_maps)
        logits, probs, bbox = self.classifier(pooled)
        mrcnn_mask = self.mask_head(self.roi_align_mask([rois, image_meta] + mrcnn_maps))
        active = active_class_ids_from_meta(image_meta)
        weights = self._loss_weights()
        total, lc, lb, lm = mrcnn_losses(target_class_ids, target_bbox, target_mask, logits, bbox, mrcnn_mask,
                                         active, weights)
        return {"loss": total, "mrcnn_class_loss": lc, "mrcnn_bbox_loss": lb, "mrcnn_mask_loss": lm,
                "rpn_rois": rpn_rois, "rois": rois, "target_gt_boxes": target_gt_boxes,
                "target_class_ids": target_class_ids, "target_bbox": target_bbox, "target_mask": target_mask,
                "mrcnn_class_logits": logits, "mrcnn_class": probs, "mrcnn_bbox": bbox, "mrcnn_mask": mrcnn_mask,
                "active_class_ids": active, "loss_weights": weights}

    def train_classifier_head(self, image, image_meta, gt_class_ids, gt_boxes, gt_masks, optimizer, seed=None):
        """One optimizer step on the classifier head (mrcnn_class_* and
        mrcnn_bbox_fc) with the reference's training-mode semantics:

          1. trunk, proposals, DetectionTargetLayer and PyramidROIAlign(POOL_SIZE)
             exactly as in head_losses, under no_grad (the trunk is frozen and runs
             on moving-statistics BN);
          2. the classifier head in training mode (batch-statistics BN over all
             ROIs, moving statistics updated with momentum 0.9);
          3. mrcnn_class_loss + mrcnn_bbox_loss (LOSS_WEIGHTS; the mask branch is
             absent);
          4. the head's backward into the ParamStore gradients;
          5. ``optimizer`` (a KerasOptimizer) on the head's chunk range, so the
             store's weight-decay term applies to the head's kernels and biases;
          6. MaxNorm on the two Dense kernels (ClassifierHead.max_norm_constraints).

        Returns a dict: "loss", "mrcnn_class_loss", "mrcnn_bbox_loss" (device
        scalars, evaluated before the update), "d_pooled" (the loss gradient with
        respect to the pooled features [B,T,p,p,p,C]) and the sampled "rois",
        "target_class_ids", "target_bbox".

        The reference's "heads" phase (TRAIN_PHASE="heads", core/models.py:
        5602-5668, 5764-5806) also leaves the RPN and the mask head trainable and
        backpropagates the head losses into every trainable layer; here only the
        classifier head moves.  d_pooled is where that backward would continue:
        its join through PyramidROIAlign's backward into the trunk is not built."""
        r = self.train_heads(image, image_meta, gt_class_ids, gt_boxes, gt_masks, optimizer, seed=seed,
                             heads=("classifier",))
        return {k: r[k] for k in ("loss", "mrcnn_class_loss", "mrcnn_bbox_loss", "d_pooled", "rois",
                                  "target_class_ids", "target_bbox")}

    def _loss_weights(self):
        """The config's LOSS_WEIGHTS of the three head losses, in LOSS_NAMES order (1 where unset)."""
        from .head_losses import LOSS_NAMES
        lw = getattr(self.config, "LOSS_WEIGHTS", {})
        return tuple(float(lw.get(n, 1.0)) for n in LOSS_NAMES)

    def train_heads(self, image, image_meta, gt_class_ids, gt_boxes, gt_masks, optimizer, seed=None,
                    heads=("classifier", "mask")):
        """One optimizer step on the selected heads with the trunk frozen (the
        head part of TRAIN_PHASE="heads", core/models.py:5602-5668):

          1. trunk, proposals, DetectionTargetLayer and PyramidROIAlign(POOL_SIZE) /
             (MASK_POOL_SIZE) under no_grad, as in head_losses;
          2. the selected heads in training mode (batch-statistics BN, moving
             statistics updated);
          3. the LOSS_WEIGHTS-weighted sum of the selected heads' losses
             (mrcnn_class_loss + mrcnn_bbox_loss for "classifier",
             mrcnn_mask_loss for "mask");
          4. backward into the ParamStore gradients of those heads;
          5. ``optimizer`` (a KerasOptimizer) on the selected heads' chunk ranges
             (one launch over both when they are adjacent in the store);
          6. MaxNorm on the two Dense kernels when the classifier is selected.

        Returns a dict: "loss" and the selected heads' losses (device scalars,
        evaluated before the update), the sampled "rois", "target_class_ids",
        "target_bbox", "target_mask", and "d_pooled" / "d_mask_pooled", the loss
        gradient with respect to the pooled features of each selected head.
        With heads=("classifier",) it is train_classifier_head.  The join of the
        two pooled gradients through PyramidROIAlign's backward into the trunk is
        not built."""
        heads = MaskRCNN._check_heads(heads, "train_heads")
        cls, msk = "classifier" in heads, "mask" in heads
        ops._dev(image, image_meta, gt_class_ids, gt_boxes, gt_masks)
        pooled = mpooled = None
        with torch.no_grad():
            _, rois, _, target_class_ids, target_bbox, target_mask, mrcnn_maps = \
                self._head_targets(image, image_meta, gt_class_ids, gt_boxes, gt_masks, seed)
            if cls:
                pooled = self.roi_align_classifier([rois, image_meta] + mrcnn_maps)
            if msk:
                mpooled = self.roi_align_mask([rois, image_meta] + mrcnn_maps)
        r = self.train_heads_on_features(pooled, mpooled, image_meta, target_class_ids, target_bbox, target_mask,
                                         optimizer, heads=heads)
        r["rois"] = rois
        return r

    @staticmethod
    def _check_heads(heads, what):
        heads = tuple(heads)
        if not heads or len(set(heads)) != len(heads) or any(h not in ("classifier", "mask") for h in heads):
            raise ValueError(f'{what}: heads must be a non-empty subset of ("classifier", "mask")')
        return heads

    def train_heads_on_features(self, rois_aligned, mask_aligned, image_meta, target_class_ids, target_bbox,
                                target_mask, optimizer, heads=("classifier", "mask")):
        """Steps 2-6 of train_heads on given ROI-aligned features: the
        HEAD_TRAINING stage's model (core/models.py:4044-4115), which takes
        rois_aligned [B,T,P,P,P,C], mask_aligned [B,T,M,M,M,C], image_meta and
        the three targets (target_class_ids [B,T] int32, target_bbox [B,T,6],
        target_mask [B,T,m,m,m]) as inputs -- a HeadGenerator item, or
        train_heads' own PyramidROIAlign results.  The features of a head that
        is not selected may be None.  Returns train_heads' dictionary without
        "rois"."""
        from . import nn as mnn
        from .head_losses import active_class_ids_from_meta, mrcnn_losses
        from .optim import apply_max_norm
        from .params import CHUNK
        heads = MaskRCNN._check_heads(heads, "train_heads_on_features")
        cls, msk = "classifier" in heads, "mask" in heads
        if (cls and rois_aligned is None) or (msk and mask_aligned is None):
            raise ValueError("train_heads_on_features: the features of a selected head are missing")
        ops._dev(rois_aligned, mask_aligned, image_meta, target_class_ids, target_bbox, target_mask)
        pooled, mpooled = rois_aligned, mask_aligned
        ranges = []
        if cls:
            pooled = pooled.detach().requires_grad_(True)
            ranges.append(self.classifier.chunk_range())
        if msk:
            mpooled = mpooled.detach().requires_grad_(True)
            ranges.append(self.mask_head.chunk_range())
        ranges.sort()
        if len(ranges) == 2:
            # one optimizer step (one step count) covers both: the heads are registered back to back
            if ranges[0][1] != ranges[1][0]:
                raise RuntimeError("train_heads: the two heads' parameters are not adjacent in the store")
            ranges = [(ranges[0][0], ranges[1][1])]
        for lo, hi in ranges:
            self.store.grad_flat[lo * CHUNK:hi * CHUNK].zero_()
        logits = bbox = mask = None
        if cls:
            logits, _, bbox = self.classifier(pooled, training=True)
        if msk:
            mask = self.mask_head(mpooled, training=True)
        total, lc, lb, lm = mrcnn_losses(target_class_ids, target_bbox if cls else None,
                                         target_mask if msk else None, logits, bbox, mask,
                                         active_class_ids_from_meta(image_meta), self._loss_weights())
        total.backward()
        mnn.join_wgrad(self.device)
        optimizer.step(self.store, chunks=ranges[0])
        if cls:
            apply_max_norm(self.store, self.classifier.max_norm_constraints)
        r = {"loss": total.detach(), "target_class_ids": target_class_ids, "target_bbox": target_bbox,
             "target_mask": target_mask}
        if cls:
            r.update(mrcnn_class_loss=lc, mrcnn_bbox_loss=lb, d_pooled=pooled.grad)
        if msk:
            r.update(mrcnn_mask_loss=lm, d_mask_pooled=mpooled.grad)
        return r

    @torch.no_grad()
    def head_target_generation(self, dataset, output_dir, split, seed=0, image_ids=None):
        """TARGET_GENERATION for one split (RPN.head_target_generation's
        ``_run_split``, core/models.py:3638-3779): for each of the first
        max(1, round(TARGET_RATIO * n)) images of ``image_ids`` (default: the
        prepared ToyDataset's) --

          * ``dataset.load_image(id, device=...)`` / ``load_data`` without
            augmentation (the generator's MODE == "targeting" branch), the
            image_meta with every class active;
          * the trunk, proposals, DetectionTargetLayer (``_head_targets``; image
            k of the split samples with seed + k) and the two PyramidROIAligns;
          * an image with fewer than MIN_POSITIVE_TARGETS (default 25) positive
            target class ids is skipped;
          * ``m3d.headstore.save_head_targets``: float16 features and bit-packed
            masks made on the device, the reference's six .npz files named by
            the image file's basename without its extension;
          * one row of paths in ``<output_dir>/datasets/<split>.csv``.

        Returns {"processed", "saved", "skipped": [(name, positives), ...],
        "csv"}.  The volume must have config.IMAGE_SHAPE (nothing is resized).
        The reference's prints and its loop that swallows every exception are
        not reproduced: an error raises."""
        import os

        from . import headstore
        from .model import compose_image_meta
        c = self.config
        shape = tuple(int(v) for v in c.IMAGE_SHAPE)
        ids = [int(i) for i in (dataset.image_ids if image_ids is None else image_ids)]
        n = max(1, int(round(float(getattr(c, "TARGET_RATIO", 1.0)) * len(ids))))
        min_positive = int(getattr(c, "MIN_POSITIVE_TARGETS", 25))
        csv_path = headstore.write_csv_header(output_dir, split)
        H, W, D = shape[:3]
        processed = saved = 0
        skipped = []
        for k, image_id in enumerate(ids[:n]):
            name = os.path.splitext(os.path.basename(str(dataset.image_info[image_id]["path"])))[0]
            image = dataset.load_image(image_id, device=self.device)
            if tuple(image.shape) != shape:
                raise ValueError(f"image {image_id} has shape {tuple(image.shape)}, the model is built for {shape} "
                                 "(head_target_generation does not resize)")
            boxes, class_ids, masks = dataset.load_data(image_id)
            meta = torch.from_numpy(compose_image_meta(image_id, shape, shape, (0, 0, 0, H, W, D), 1.0,
                                                       np.ones(c.NUM_CLASSES, np.int32))[None]).to(self.device)
            _, rois, _, tci, tbox, tmask, maps = self._head_targets(
                image[None], meta, torch.from_numpy(np.asarray(class_ids, np.int32)[None]).to(self.device),
                torch.from_numpy(np.asarray(boxes, np.float32).reshape(1, -1, 6)).to(self.device),
                torch.from_numpy(np.ascontiguousarray(masks != 0)[None]).to(self.device), seed + k)
            pooled = self.roi_align_classifier([rois, meta] + maps)
            mpooled = self.roi_align_mask([rois, meta] + maps)
            processed += 1
            positives = int((tci > 0).sum())
            if positives < min_positive:
                skipped.append((name, positives))
                continue
            paths = headstore.save_head_targets(output_dir, name, rois[0], pooled[0], mpooled[0], tci[0], tbox[0],
                                                tmask[0])
            headstore.append_csv_row(csv_path, paths)
            saved += 1
        return {"processed": processed, "saved": saved, "skipped": skipped, "csv": csv_path}

    def load_weights(self, filepath, by_name=True, skip_mismatch=False, exclude=()):
        """keras_model.load_weights(filepath, by_name=True, ...) on the Keras-H5 format (m3d.weights)."""
        from .weights import load_weights
        return load_weights(self.store, filepath, by_name=by_name, skip_mismatch=skip_mismatch, exclude=exclude)

    def save_weights(self, filepath):
        """keras_model.save_weights(filepath): Keras-H5 layout, readable by the reference."""
        from .weights import save_weights
        save_weights(self.store, filepath)

    @torch.no_grad()
    def detect(self, image, image_meta):
        _, C2, C3, C4, C5 = self.backbone(image)
        fmaps = self.fpn(C2, C3, C4, C5)
        _, rpn_probs, rpn_bbox = self.rpn(fmaps)
        rpn_rois = self.proposal_layer([rpn_probs, rpn_bbox, self.anchors])
        mrcnn_maps = fmaps[:4]
        pooled = self.roi_align_classifier([rpn_rois, image_meta] + mrcnn_maps)
        _, mrcnn_class, mrcnn_bbox = self.classifier(pooled)
        detections = self.detection([rpn_rois, mrcnn_class, mrcnn_bbox, image_meta])
        mpooled = self.roi_align_mask([detections[..., :6].contiguous(), image_meta] + mrcnn_maps)
        mrcnn_mask = self.mask_head(mpooled)
        return {"detections": detections, "mrcnn_class": mrcnn_class, "mrcnn_bbox": mrcnn_bbox,
                "mrcnn_mask": mrcnn_mask, "rpn_rois": rpn_rois, "feature_maps": fmaps,
                "pooled": pooled, "mask_pooled": mpooled, "rpn_class": rpn_probs, "rpn_bbox": rpn_bbox}

    @torch.no_grad()
    def evaluate(self, image, image_meta, gt_class_ids, gt_boxes, gt_masks, iou_threshold=0.5, labels=False):
        """The reference's MRCNN_EVALUATION for one image [1,H,W,D,Cin]: detect ->
        unmold_detections -> mask overlaps against gt_masks [H,W,D,G] (or
        [1,H,W,D,G]; uint8, G innermost) -> compute_ap (m3d.evaluate).  Returns
        evaluate_detections' dict (mAP, precision, recall, ious, iou, ...) plus
        ``detections`` and ``mrcnn_mask``.  gt_boxes is accepted for the
        reference's signature; the mask IoU does not read it.  ``labels``: also
        the instance label volume and the pixelwise / Dice / detection metrics
        (evaluate_detections)."""
        from .evaluate import evaluate_detections
        ops._dev(image, image_meta, gt_masks)
        if image.shape[0] != 1:
            raise ValueError("MaskRCNN.evaluate takes one image; loop over a batch")
        r = self.detect(image, image_meta)
        if torch.is_tensor(gt_class_ids) and gt_class_ids.dim() == 2:
            gt_class_ids = gt_class_ids[0]
        out = evaluate_detections(r["detections"][0], r["mrcnn_mask"][0], tuple(image.shape[1:4]), gt_class_ids,
                                  gt_masks, iou_threshold, labels=labels)
        out["detections"], out["mrcnn_mask"] = r["detections"], r["mrcnn_mask"]
        return out

    @torch.no_grad()
    def evaluate_dataset(self, dataset, result_dir=None, image_ids=None, iou_threshold=0.5):
        """The reference's MRCNN_EVALUATION loop over a prepared ToyDataset
        (core/models.py:7165-7196 with the per-image report of 6099-6151): per
        image load_image / load_data (the volume must have config.IMAGE_SHAPE:
        nothing is resized), evaluate(labels=True), and with ``result_dir`` the
        segmentation volume ``<name>.tiff`` ([D,H,W] pages of instance labels,
        uint8 up to 255 detections, else uint16) and ``<name>.csv`` (class and
        pixel box of each listed detection, in label order); ``name`` is the
        image file's basename without its extension.  Returns {"rows": one
        report dict per image, "summary": mean / std of the pixelwise F1 and of
        the instance Dice, mean mask-level recall / precision, over the
        images}.  The label stack is copied to the host once per image, only
        when ``result_dir`` is set."""
        import os

        from .evaluate import write_detection_csv
        from .model import compose_image_meta
        from .tiff import imwrite
        shape = tuple(int(v) for v in self.config.IMAGE_SHAPE)
        if result_dir is not None:
            os.makedirs(result_dir, exist_ok=True)
        rows = []
        for image_id in (dataset.image_ids if image_ids is None else image_ids):
            image_id = int(image_id)
            image = dataset.load_image(image_id)
            if tuple(image.shape) != shape:
                raise ValueError(f"image {image_id} has shape {tuple(image.shape)}, the model is built for {shape} "
                                 "(evaluate_dataset does not resize)")
            _, class_ids, masks = dataset.load_data(image_id)
            H, W, D = shape[:3]
            meta = compose_image_meta(image_id, shape, shape, (0, 0, 0, H, W, D), 1.0,
                                      np.ones(self.config.NUM_CLASSES, np.int32))
            out = self.evaluate(torch.from_numpy(image[None]).to(self.device),
                                torch.from_numpy(meta[None]).to(self.device), class_ids.astype(np.int32), None,
                                torch.from_numpy(np.ascontiguousarray(masks != 0).view(np.uint8)).to(self.device),
                                iou_threshold, labels=True)
            name = os.path.splitext(os.path.basename(str(dataset.image_info[image_id]["path"])))[0]
            if result_dir is not None:
                imwrite(os.path.join(result_dir, name + ".tiff"), out["unmolded"].label_stack().cpu().numpy())
                write_detection_csv(os.path.join(result_dir, name + ".csv"), out["class_ids"], out["boxes"])
            n_pred, n_gt = len(out["rows"]), masks.shape[-1]
            row = {"name": name, "pred_inst": n_pred}
            if n_gt == 0 and n_pred == 0:                       # the reference's all-zero report
                row.update(ap50=0.0, prec50=0.0, rec50=0.0, miou=0.0)
            else:
                ious = np.asarray(out["ious"], np.float32)
                row.update(ap50=float(out["mAP"]), prec50=float(out["precision"]), rec50=float(out["recall"]),
                           miou=float(np.nanmean(ious)) if ious.size else 0.0)
            px, dice, det = out["pixelwise"], out["instance_dice"], out["detection_performance"]
            row.update(px_precision=px[0], px_recall=px[1], px_f1=px[2], px_iou=px[3], dice_mean=dice[0],
                       dice_std=dice[1], dice_n=dice[2], det_tp=det["tp"], det_fp=det["fp"], det_fn=det["fn"],
                       det_recall=det["recall"], det_precision=det["precision"])
            rows.append(row)

        def stat(fn, key):
            return float(fn([r[key] for r in rows])) if rows else 0.0
        summary = {"images": len(rows), "pixelwise_f1_mean": stat(np.mean, "px_f1"),
                   "pixelwise_f1_std": stat(np.std, "px_f1"), "instance_dice_mean": stat(np.mean, "dice_mean"),
                   "instance_dice_std": stat(np.std, "dice_mean"), "recall_mean": stat(np.mean, "det_recall"),
                   "precision_mean": stat(np.mean, "det_precision")}
        return {"rows": rows, "summary": summary}
