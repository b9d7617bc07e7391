"""The three Mask R-CNN head losses on libm3d (csrc/head_loss.hip).

``mrcnn_losses(target_class_ids, target_bbox, target_mask, mrcnn_class_logits,
mrcnn_bbox, mrcnn_mask, active_class_ids)`` -> (total, class_loss, bbox_loss,
mask_loss): mrcnn_class_loss_graph (core/models.py:1676-1807),
mrcnn_bbox_loss_graph (1810-1877) and mrcnn_mask_loss_graph (1881-1960) in one
fused forward (m3d_head_loss_fwd) with their gradients w.r.t. the three head
outputs in one fused backward (m3d_head_loss_bwd).  It sits between
DetectionTargetLayer's outputs ([B,T] int32 class ids, [B,T,6] deltas,
[B,T,mh,mw,md] masks) and the heads' ([B,T,C] logits, [B,T,C,6] boxes,
[B,T,mh,mw,md,C] masks) and takes both as they come.  ``mrcnn_class_loss`` /
``mrcnn_bbox_loss`` / ``mrcnn_mask_loss`` are the single losses with the
reference's argument order.  GPU only: there is no CPU fallback.
"""
from __future__ import annotations

import torch

from . import _lib, ops
from .config import DEFAULTS

LOSS_NAMES = ("mrcnn_class_loss", "mrcnn_bbox_loss", "mrcnn_mask_loss")


def active_class_ids_from_meta(image_meta):
    """parse_image_meta_graph(meta)["active_class_ids"] (core/models.py:7524)."""
    return image_meta[:, 16:]


class _HeadLossFused(torch.autograd.Function):
    """The losses present (a None prediction skips its branch) and their
    weighted total in at most three launches; the backward writes the three
    gradients whole in at most two.  The forward does no gradient work."""

    @staticmethod
    def forward(ctx, logits, bbox, mask, ids, tbox, tmask, active, B, T, C, V, alpha, gamma, w):
        dev = ids.device
        L = _lib.load()
        R = B * T
        total, lc, lb, lm = (torch.empty((), device=dev, dtype=torch.float32) for _ in range(4))
        state = torch.empty(4 + 4 * R, device=dev, dtype=torch.float32)
        ws = torch.empty(max(int(L.m3d_head_loss_workspace_bytes(R, V)), 16), device=dev, dtype=torch.uint8)
        p = _lib.ptr
        _lib.check(L.m3d_head_loss_fwd(p(logits), p(bbox), p(mask), p(ids), p(tbox), p(tmask), p(active), B, T, C, V,
                                       alpha, gamma, w[0], w[1], w[2], p(total), p(lc), p(lb), p(lm), p(state), p(ws),
                                       ws.numel(), _lib.stream()), "m3d_head_loss_fwd")
        ctx.save_for_backward(logits, bbox, mask, ids, tbox, tmask, active, state)
        ctx.dims = (B, T, C, V, alpha, gamma)
        ctx.mark_non_differentiable(lc, lb, lm)
        return total, lc, lb, lm

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_total, _g_lc, _g_lb, _g_lm):
        logits, bbox, mask, ids, tbox, tmask, active, state = ctx.saved_tensors
        B, T, C, V, alpha, gamma = ctx.dims
        need = ctx.needs_input_grad
        if g_total is None:
            return (None,) * 14
        g_total = g_total.contiguous().to(torch.float32)
        g_logits = torch.empty_like(logits) if logits is not None and need[0] else None
        g_bbox = torch.empty_like(bbox) if bbox is not None and need[1] else None
        g_mask = torch.empty_like(mask) if mask is not None and need[2] else None   # written whole: no memset
        p = _lib.ptr
        _lib.check(_lib.load().m3d_head_loss_bwd(p(logits), p(bbox), p(mask), p(ids), p(tbox), p(tmask), p(active),
                                                 B, T, C, V, alpha, gamma, p(state), p(g_total), p(g_logits),
                                                 p(g_bbox), p(g_mask), _lib.stream()), "m3d_head_loss_bwd")
        return (g_logits, g_bbox, g_mask) + (None,) * 11


def _f32(t):
    return None if t is None else ops._c(t)


def mrcnn_losses(target_class_ids, target_bbox, target_mask, mrcnn_class_logits, mrcnn_bbox, mrcnn_mask,
                 active_class_ids, weights=None, alpha=0.85, gamma=3.0):
    """(total, mrcnn_class_loss, mrcnn_bbox_loss, mrcnn_mask_loss), four device
    scalars; total = the LOSS_WEIGHTS-weighted sum and the only one carrying
    gradient.  ``weights``: (class, bbox, mask), default the config's
    LOSS_WEIGHTS entries (1.0 each).  target_mask may carry the reference's
    trailing 1 axis.  A None prediction skips that loss (its value is 0):
    MaskRCNN evaluates class + bbox and mask at different ROI counts."""
    ops._dev(target_class_ids, target_bbox, target_mask, mrcnn_class_logits, mrcnn_bbox, mrcnn_mask,
             active_class_ids)
    if target_class_ids.dim() == 3 and target_class_ids.shape[-1] == 1:
        target_class_ids = target_class_ids[..., 0]
    if target_class_ids.dim() != 2:
        raise ValueError("target_class_ids must be [B,T]")
    B, T = (int(v) for v in target_class_ids.shape)
    preds = [t for t in (mrcnn_class_logits, mrcnn_bbox, mrcnn_mask) if t is not None]
    if not preds:
        raise ValueError("mrcnn_losses: no prediction given")
    C = int(mrcnn_mask.shape[-1] if mrcnn_class_logits is None and mrcnn_bbox is None else
            (mrcnn_class_logits.shape[-1] if mrcnn_class_logits is not None else mrcnn_bbox.shape[-2]))
    V = 0
    if mrcnn_class_logits is not None and tuple(mrcnn_class_logits.shape) != (B, T, C):
        raise ValueError(f"mrcnn_class_logits must be [B,T,C] = {(B, T, C)}, got {tuple(mrcnn_class_logits.shape)}")
    if mrcnn_bbox is not None:
        if tuple(mrcnn_bbox.shape) != (B, T, C, 6) or target_bbox is None or tuple(target_bbox.shape) != (B, T, 6):
            raise ValueError("mrcnn_bbox must be [B,T,C,6] and target_bbox [B,T,6]")
    if mrcnn_mask is not None:
        if mrcnn_mask.dim() != 6 or tuple(mrcnn_mask.shape[:2]) != (B, T) or mrcnn_mask.shape[-1] != C:
            raise ValueError("mrcnn_mask must be [B,T,mh,mw,md,C]")
        ms = tuple(mrcnn_mask.shape[2:5])
        if target_mask is not None and target_mask.dim() == 6 and target_mask.shape[-1] == 1:
            target_mask = target_mask[..., 0]
        if target_mask is None or tuple(target_mask.shape) != (B, T) + ms:
            raise ValueError("target_mask must be [B,T,mh,mw,md] like mrcnn_mask")
        V = int(ms[0] * ms[1] * ms[2])
    if active_class_ids is not None and tuple(active_class_ids.shape) != (B, C):
        raise ValueError(f"active_class_ids must be [B,C] = {(B, C)}, got {tuple(active_class_ids.shape)}")
    if weights is None:
        weights = tuple(float(DEFAULTS["LOSS_WEIGHTS"][n]) for n in LOSS_NAMES)
    elif isinstance(weights, dict):
        weights = tuple(float(weights[n]) for n in LOSS_NAMES)
    w = tuple(float(v) for v in weights)
    if len(w) != 3:
        raise ValueError("weights: (class, bbox, mask)")
    ids = target_class_ids.detach().to(torch.int32).contiguous()
    tbox = _f32(target_bbox.detach()) if mrcnn_bbox is not None else None
    tmask = _f32(target_mask.detach()) if mrcnn_mask is not None else None
    active = _f32(active_class_ids.detach()) if active_class_ids is not None else None
    return _HeadLossFused.apply(_f32(mrcnn_class_logits), _f32(mrcnn_bbox), _f32(mrcnn_mask), ids, tbox, tmask,
                                active, B, T, C, V, float(alpha), float(gamma), w)


def mrcnn_class_loss(target_class_ids, pred_class_logits, active_class_ids, alpha=0.85, gamma=3.0):
    """mrcnn_class_loss_graph(target_class_ids, pred_class_logits, active_class_ids)."""
    return mrcnn_losses(target_class_ids, None, None, pred_class_logits, None, None, active_class_ids,
                        (1.0, 0.0, 0.0), alpha, gamma)[0]


def mrcnn_bbox_loss(target_bbox, target_class_ids, pred_bbox):
    """mrcnn_bbox_loss_graph(target_bbox, target_class_ids, pred_bbox)."""
    return mrcnn_losses(target_class_ids, target_bbox, None, None, pred_bbox, None, None, (0.0, 1.0, 0.0))[0]


def mrcnn_mask_loss(target_masks, target_class_ids, pred_masks):
    """mrcnn_mask_loss_graph(target_masks, target_class_ids, pred_masks)."""
    return mrcnn_losses(target_class_ids, None, target_masks, None, None, pred_masks, None, (0.0, 0.0, 1.0))[0]
