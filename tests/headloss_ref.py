"""Torch restatement of the reference's three head-loss graphs, written from
core/models.py line by line (the debug prints and diagnostics left out):

  class_loss  mrcnn_class_loss_graph  core/models.py:1676-1807
  bbox_loss   mrcnn_bbox_loss_graph   core/models.py:1810-1877
  mask_loss   mrcnn_mask_loss_graph   core/models.py:1881-1960

dtype- and device-generic: the predictions' dtype and device are used
throughout.  CPU float64 is the checker of the fused kernels
(tests/test_gpu_head_loss.py); float32 on the GPU is the framework-op timing
baseline (scripts/time_head_loss.py).  Gradients come from autograd.

The clip constants are the float32-rounded values the float32 graph uses
(K.epsilon() = float32(1e-7), 1 - K.epsilon() rounded to float32, alpha cast to
float32), so a value placed on a boundary falls on the same side in both
precisions.
"""
import numpy as np
import torch

EPS = float(np.float32(1e-7))
ONE_MINUS_EPS = float(np.float32(1.0) - np.float32(1e-7))


def _f32(v):
    return float(np.float32(v))


def class_loss(target_class_ids, pred_class_logits, active_class_ids, alpha=0.85, gamma=3.0):
    x = pred_class_logits
    dt = x.dtype
    B, T, C = x.shape
    active = active_class_ids.to(dt)
    active = torch.cat([torch.ones_like(active[..., :1]), active[..., 1:]], dim=-1)      # :1692
    logits = x.clamp(-10.0, 10.0)                                                       # :1697
    logits_flat = logits.reshape(B * T, C)
    target_flat = target_class_ids.reshape(B * T).long()
    # tf.tile(active, [T, 1]) -> [T*B, C]: row r is active[r mod B] (:1702-1705)
    active_repeated = active.repeat(T, 1)
    row_idx = torch.arange(B * T, device=x.device)
    true_active = active_repeated[row_idx, target_flat]
    probs_flat = torch.softmax(logits_flat, dim=-1)                                      # :1708
    pt = probs_flat[row_idx, target_flat].clamp(EPS, ONE_MINUS_EPS)                      # :1711-1712
    alpha, gamma = _f32(alpha), _f32(gamma)
    focal_weight = (1.0 - pt) ** gamma                                                   # :1717
    ce = torch.logsumexp(logits_flat, dim=-1) - logits_flat[row_idx, target_flat]        # :1718
    focal_loss = focal_weight * ce
    is_fg = (target_flat > 0).to(dt)
    class_weights = is_fg * alpha + (1.0 - is_fg) * (1.0 - alpha)                        # :1722-1724
    max_fg_prob = probs_flat[:, 1:].max(dim=-1).values                                   # :1728-1729
    is_confident_fp = ((target_flat == 0) & (max_fg_prob > 0.5)).to(dt)                  # :1737-1740
    focal_loss = focal_loss * (1.0 + is_confident_fp * (2.0 - 1.0))                      # :1743-1744
    focal_loss = focal_loss * class_weights * true_active                               # :1747
    weight_sum = (class_weights * true_active).sum()                                     # :1805
    denom = torch.clamp(weight_sum.detach(), min=EPS)
    return focal_loss.sum() / denom


def bbox_loss(target_bbox, target_class_ids, pred_bbox):
    dt = pred_bbox.dtype
    y_true = target_bbox.reshape(-1, 6).to(dt)
    cls = target_class_ids.reshape(-1).long()
    y_pred = pred_bbox.reshape(y_true.shape[0], -1, 6)
    pos_ix = torch.nonzero(cls > 0)[:, 0]                                                # :1825
    if pos_ix.numel() == 0:
        return pred_bbox.sum() * 0.0                                                     # _no_pos
    yt = y_true[pos_ix]
    yp_cls = y_pred[pos_ix, cls[pos_ix]]                                                 # :1836-1837
    yp_cls = 3.0 * torch.tanh(yp_cls / 3.0)                                              # :1841
    abs_diff = (yt - yp_cls).abs()
    huber = torch.where(abs_diff <= 1.0, 0.5 * abs_diff * abs_diff, abs_diff - 0.5)      # :1848-1852
    return huber.mean(dim=-1).mean()                                                     # :1855-1856


def mask_loss(target_masks, target_class_ids, pred_masks):
    dt = pred_masks.dtype
    B, T = target_masks.shape[:2]
    C = pred_masks.shape[-1]
    V = int(np.prod(pred_masks.shape[2:5]))
    y_true = target_masks.reshape(B * T, V).to(dt)
    y_pred = pred_masks.reshape(B * T, V, C)
    cls1d = target_class_ids.reshape(B * T).long()
    pos_ix = torch.nonzero(cls1d > 0)[:, 0]
    zero = pred_masks.sum() * 0.0
    if pos_ix.numel() == 0:
        return zero                                                                     # _no_pos
    yt = y_true[pos_ix]
    yp_t = y_pred[pos_ix].permute(0, 2, 1)                                               # [P,C,V]
    yp_cls = yp_t[torch.arange(pos_ix.numel(), device=pos_ix.device), cls1d[pos_ix]]     # [P,V]
    yp_prob = yp_cls.clamp(EPS, ONE_MINUS_EPS)                                           # :1906
    valid = yt.sum(dim=-1) > 0                                                           # :1909
    yt, yp_prob = yt[valid], yp_prob[valid]
    if yt.shape[0] == 0:
        return zero                                                                     # _no_valid
    # K.binary_crossentropy(target, output) of TF 2.2 on probabilities
    out = yp_prob.clamp(EPS, ONE_MINUS_EPS)
    bce = -(yt * torch.log(out + EPS) + (1.0 - yt) * torch.log(1.0 - out + EPS))
    bce_loss = bce.mean()                                                                # :1917
    inter = (yt * yp_prob).sum(dim=-1)
    union = yt.sum(dim=-1) + yp_prob.sum(dim=-1)
    dice = (2.0 * inter + 1.0) / (union + 1.0)                                           # :1918-1921
    return 0.3 * bce_loss + 0.7 * (1.0 - dice.mean())                                    # :1922-1923


def losses(target_class_ids, target_bbox, target_mask, class_logits, bbox, mask, active_class_ids,
           weights=(1.0, 1.0, 1.0), alpha=0.85, gamma=3.0):
    """(total, class, bbox, mask): the three graphs and their weighted sum."""
    lc = class_loss(target_class_ids, class_logits, active_class_ids, alpha, gamma)
    lb = bbox_loss(target_bbox, target_class_ids, bbox)
    lm = mask_loss(target_mask, target_class_ids, mask)
    return lc * weights[0] + lb * weights[1] + lm * weights[2], lc, lb, lm
