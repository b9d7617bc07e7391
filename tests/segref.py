"""numpy restatement of the segmentation volume and the per-image metrics of
the reference's MRCNN_EVALUATION, built on the dense masks of
tests/unmoldref.py (``U.unmold(...)["dense"]``):

* the label loop ``seg[full > 0.5] = j + 1`` over the kept list
  (core/models.py:7023-7069): a rejected mask is all zero, so it consumes its
  label and paints nothing; the later detection wins a shared voxel;
* the pixelwise counts and metrics (_pixelwise_metrics, 6153-6164);
* the two greedy matchings in the reference's dense form, ``P.T @ T`` on the
  flattened masks: the instance Dice (_instance_dice, 6166-6282) and the
  mask-level detection counts (_compute_mask_metrics, 6663-6706).

tests/test_segref.py pins this file with hand-derived answers and holds
m3d.evaluate's host functions against it; tests/test_gpu_segment.py compares
the kernels with it.
"""
import numpy as np

import unmoldref as U


def listed_rows(status, keep=None):
    """The rows that get a label: kept by the unmolding (status != NOT_KEPT)
    and, with ``keep``, not dropped by the caller."""
    listed = np.asarray(status) != U.NOT_KEPT
    if keep is not None:
        listed &= np.asarray(keep) != 0
    return np.flatnonzero(listed)


def labels(dense, status, keep=None):
    """dense [N,H,W,D] uint8 (all zero for a rejected row), status [N] ->
    (seg [H,W,D] int32, label_of [N] int32)."""
    seg = np.zeros(dense.shape[1:], np.int32)
    label_of = np.zeros(len(status), np.int32)
    for k, row in enumerate(listed_rows(status, keep)):
        label_of[row] = k + 1
        seg[dense[row] > 0] = k + 1
    return seg, label_of


def pixelwise_counts(seg, gt_masks):
    """(tp, fp, fn) of (seg > 0) against (any GT mask set); gt_masks [H,W,D,G]."""
    pred_bin = seg > 0
    gt_bin = (np.asarray(gt_masks) > 0).any(axis=-1)
    tp = np.logical_and(pred_bin, gt_bin).sum(dtype=np.int64)
    fp = np.logical_and(pred_bin, np.logical_not(gt_bin)).sum(dtype=np.int64)
    fn = np.logical_and(np.logical_not(pred_bin), gt_bin).sum(dtype=np.int64)
    return int(tp), int(fp), int(fn)


def pixelwise_metrics(tp, fp, fn):
    tp, fp, fn = np.int64(tp), np.int64(fp), np.int64(fn)
    prec = (tp / (tp + fp + 1e-9)) if (tp + fp) > 0 else 0.0
    rec = (tp / (tp + fn + 1e-9)) if (tp + fn) > 0 else 0.0
    f1 = (2.0 * prec * rec / (prec + rec + 1e-9)) if (prec + rec) > 0 else 0.0
    iou = (tp / (tp + fp + fn + 1e-9)) if (tp + fp + fn) > 0 else 0.0
    return float(prec), float(rec), float(f1), float(iou)


def _flat(pred_masks, gt_masks):
    """pred_masks [H,W,D,K], gt_masks [H,W,D,G] -> P [V,K], T [V,G] bool."""
    K, G = pred_masks.shape[-1], gt_masks.shape[-1]
    return (np.asarray(pred_masks) > 0).reshape(-1, K), (np.asarray(gt_masks) > 0).reshape(-1, G)


def _counts(P, T):
    p_sum = P.sum(axis=0).astype(np.int64)
    t_sum = T.sum(axis=0).astype(np.int64)
    inter = (P.T.astype(np.float64) @ T.astype(np.float64)).astype(np.int64)    # counts < 2^53: exact
    return inter, p_sum, t_sum


def instance_dice(pred_masks, gt_masks, iou_thr=0.5):
    """(mean, std, n) over the greedily matched pairs."""
    K, G = pred_masks.shape[-1], gt_masks.shape[-1]
    if K == 0 or G == 0:
        return 0.0, 0.0, 0
    inter, p_sum, t_sum = _counts(*_flat(pred_masks, gt_masks))
    union = (p_sum[:, None] + t_sum[None, :]) - inter
    iou = inter / np.maximum(union, 1)
    used_p = np.zeros((K,), dtype=np.bool_)
    used_g = np.zeros((G,), dtype=np.bool_)
    dices = []
    while True:
        iou_mask = iou.copy()
        iou_mask[used_p, :] = -1.0
        iou_mask[:, used_g] = -1.0
        k, g = np.unravel_index(np.argmax(iou_mask), iou_mask.shape)
        if iou_mask[k, g] < iou_thr:
            break
        denom = p_sum[k] + t_sum[g]
        d = (2.0 * inter[k, g] / denom) if denom > 0 else 0.0
        dices.append(float(d))
        used_p[k] = True
        used_g[g] = True
    if len(dices) == 0:
        return 0.0, 0.0, 0
    return float(np.mean(dices)), float(np.std(dices)), int(len(dices))


def detection_performance(pred_masks, gt_masks, thr=0.5):
    """tp / fp / fn / recall / precision of the second greedy loop.  Without
    predictions or ground truths nothing can match: all fp / all fn."""
    n_pred, n_gt = pred_masks.shape[-1], gt_masks.shape[-1]
    matched_pred = np.zeros(n_pred, dtype=bool)
    matched_gt = np.zeros(n_gt, dtype=bool)
    if n_pred > 0 and n_gt > 0:
        intersection, pd_sum, gt_sum = _counts(*_flat(pred_masks, gt_masks))
        union = pd_sum[:, None] + gt_sum[None, :] - intersection
        mask_ious = intersection / np.maximum(union, 1)
        while True:
            best_i, best_j = np.unravel_index(np.argmax(mask_ious), mask_ious.shape)
            if mask_ious[best_i, best_j] < thr:
                break
            matched_pred[best_i] = True
            matched_gt[best_j] = True
            mask_ious[best_i, :] = 0
            mask_ious[:, best_j] = 0
    tp = np.sum(matched_pred)
    fp = n_pred - tp
    fn = n_gt - np.sum(matched_gt)
    return {"tp": int(tp), "fp": int(fp), "fn": int(fn),
            "recall": float(tp / (tp + fn)) if (tp + fn) > 0 else 0.0,
            "precision": float(tp / (tp + fp)) if (tp + fp) > 0 else 0.0}


def listed_masks(dense, status, keep=None):
    """[H,W,D,K]: the dense masks of the listed rows, in label order."""
    return np.moveaxis(np.asarray(dense)[listed_rows(status, keep)], 0, -1)
