"""RPN evaluation on libm3d (csrc/rpn_eval.hip): the reference's RPN_EVALUATION
chain RPN.evaluate (core/models.py:3799-3806) -> RPNEvaluationCallback
(2165-2209) -> rpn_evaluation (core/utils.py:1251-1415) without its per-image
copy of the proposals to the host.

``score_proposals`` scores one image's ``rpn_rois`` against its ground-truth
pixel boxes on the device and leaves a small integer record there: which
proposal claimed each GT box among the first ``EVAL_TOPK_RPN`` rows, that
proposal's pixel box, and for every threshold of ``EVAL_MATCH_IOU_GRID`` the
first row that reaches it (from which the hit count of every prefix of
``EVAL_TOPK_GRID`` follows).  ``summarize`` turns a subset's records and losses
into the callback's numbers on the host, in NumPy.  ``RPN.evaluate``
(m3d.model) is the loop: one synchronising copy per subset.  GPU only: there
is no CPU fallback.

The record of one image is one int32 row, packed by that image's G:

    counts [2] | assoc [G] | matched [G,6] (float32 bits) | first_hit [T,G]

``record_len(G, T)`` is its length and ``unpack_record`` its host view.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, ops

MAX_GT = 512                # m3d_rpn_eval_proposals: the GT boxes are staged in LDS
MAX_GRID = 8

_GRIDS = {}                 # (device, thresholds) -> device float32 tensor


def record_len(G, T):
    return 2 + int(G) * (7 + int(T))


def _grid_tensor(iou_grid, device):
    if torch.is_tensor(iou_grid):
        ops._dev(iou_grid)
        return ops._c(iou_grid.reshape(-1))
    vals = tuple(float(np.float32(v)) for v in iou_grid)
    key = (str(device), vals)
    if key not in _GRIDS:
        _GRIDS[key] = torch.tensor(vals, dtype=torch.float32, device=device)
    return _GRIDS[key]


def score_proposals(rois, gt_boxes, shape, topk, match_iou, iou_grid, out=None, return_iou=False):
    """rois [R,6] (or [1,R,6]) normalised proposals, gt_boxes [G,6] float32
    pixel boxes, both on the GPU; ``shape`` (H,W,D); ``topk`` = EVAL_TOPK_RPN,
    ``match_iou`` = EVAL_MATCH_IOU (a Python float: the compare is in double),
    ``iou_grid`` = EVAL_MATCH_IOU_GRID (a sequence, uploaded once per device, or
    a device float32 tensor) -> the device record, int32 [record_len(G, T)].

    ``out``: an int32 device tensor to write the record into, e.g. row k of a
    preallocated [steps, width] buffer (contiguous, at least record_len(G, T)
    long); the returned record is its leading part.  ``return_iou``: also
    return the [G,R] float32 IoU matrix (0 for invalid rows).  Nothing
    synchronises.  G == 0 is the caller's case (the reference reports only the
    losses for such an image): it raises here."""
    ops._dev(rois, gt_boxes, out)
    if rois.dim() == 3 and rois.shape[0] == 1:
        rois = rois[0]
    if rois.dim() != 2 or rois.shape[1] != 6:
        raise ValueError(f"rois must be [R,6], got {tuple(rois.shape)}")
    if gt_boxes.dim() != 2 or gt_boxes.shape[1] != 6:
        raise ValueError(f"gt_boxes must be [G,6], got {tuple(gt_boxes.shape)}")
    R, G = int(rois.shape[0]), int(gt_boxes.shape[0])
    if G < 1 or G > MAX_GT:
        raise ValueError(f"score_proposals takes 1 .. {MAX_GT} GT boxes, got {G} (an image without GT is not scored)")
    H, W, D = (int(v) for v in tuple(shape)[:3])
    grid = _grid_tensor(iou_grid, rois.device)
    T = int(grid.numel())
    if T > MAX_GRID:
        raise ValueError(f"at most {MAX_GRID} IoU thresholds, got {T}")
    n = record_len(G, T)
    if out is None:
        out = torch.empty(n, device=rois.device, dtype=torch.int32)
    elif out.dtype != torch.int32 or out.dim() != 1 or out.numel() < n or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous int32 tensor of at least {n} elements, got {out.dtype} "
                         f"{tuple(out.shape)}")
    rec = out[:n]
    rois, gt = ops._c(rois.detach()), ops._c(gt_boxes.detach())
    iou = torch.empty((G, R), device=rois.device, dtype=torch.float32) if return_iou else None
    p, base = _lib.ptr, rec.data_ptr()
    _lib.check(_lib.load().m3d_rpn_eval_proposals(
        p(rois) if R else None, R, p(gt), G, H, W, D, int(topk), float(match_iou), p(grid) if T else None, T,
        base + 8, base + 4 * (2 + G), (base + 4 * (2 + 7 * G)) if T else None, base, p(iou) if R else None,
        _lib.stream()), "m3d_rpn_eval_proposals")
    return (rec, iou) if return_iou else rec


def unpack_record(row, G, T):
    """A host int32 row (or a longer buffer row) -> dict of views: ``counts``
    [2], ``assoc`` [G], ``matched`` [G,6] float32, ``first_hit`` [T,G]."""
    row = np.ascontiguousarray(np.asarray(row, np.int32).reshape(-1)[:record_len(G, T)])
    return {"counts": row[:2], "assoc": row[2:2 + G],
            "matched": row[2 + G:2 + 7 * G].view(np.float32).reshape(G, 6),
            "first_hit": row[2 + 7 * G:].reshape(T, G)}


def _mean(v):
    return float(np.mean(v)) if len(v) else 0.0


def _std(v):
    return float(np.std(v)) if len(v) else 0.0


def summarize(records, class_losses, bbox_losses, gt_boxes_per_image, topk_grid, iou_grid, subset="test"):
    """The numbers of one subset, on the host (core/utils.py:1257-1415).

    ``records[i]`` is image i's record as a dict (``unpack_record``, or the
    restatement's) or its int32 row, or None for an image that was not scored;
    ``gt_boxes_per_image[i]`` its [G,6] pixel boxes; the losses are one float
    per image.  Per image, as there: the losses always count; without GT, or
    without a valid ROI among the first EVAL_TOPK_RPN rows, nothing else does;
    Detection@thr@K = 100 #{g: first_hit[t,g] < K} / max(1, G) for every K
    whose prefix holds a valid row; without a match the detection score is 0
    and no coordinate error is recorded; otherwise the coordinate error is
    mean(|matched - gt|) over the matched pairs in GT order, in float64, and
    the score 100 matched / G.  Means and stds of empty lists are 0.

    -> {rpn_<subset>_class_mean, _class_std, _bbox_mean, _bbox_std,
    _mean_coord_error, _detection_score, detection_at: {"0.30@500": mean, ...}}
    (a Detection@ key no image contributed to is absent)."""
    thrs = [float(t) for t in iou_grid]
    T = len(thrs)
    class_loss, bbox_loss, errors, scores, det_at = [], [], [], [], {}
    for i, gt in enumerate(gt_boxes_per_image):
        class_loss.append(float(class_losses[i]))
        bbox_loss.append(float(bbox_losses[i]))
        gt = np.zeros((0, 6), np.float32) if gt is None else np.asarray(gt).reshape(-1, 6)
        G = gt.shape[0]
        rec = records[i]
        if G == 0 or rec is None:
            continue
        if not isinstance(rec, dict):
            rec = unpack_record(rec, G, T)
        counts, assoc = np.asarray(rec["counts"]), np.asarray(rec["assoc"])
        if int(counts[0]) == 0:
            continue
        first_hit = np.asarray(rec["first_hit"]).reshape(T, G)
        for K in topk_grid:
            if int(counts[1]) >= int(K):
                continue
            for t, thr in enumerate(thrs):
                hits = int((first_hit[t] < int(K)).sum())
                det_at.setdefault(f"{thr:.2f}@{int(K)}", []).append(100.0 * float(hits) / max(1, G))
        hit = assoc >= 0
        if not hit.any():
            scores.append(0.0)
            continue
        diff = np.asarray(rec["matched"], np.float32)[hit].astype(np.float64) - gt[hit].astype(np.float64)
        errors.append(float(np.mean(np.abs(diff))))
        scores.append(100.0 * int(hit.sum()) / max(1, G))
    k = f"rpn_{subset}_"
    return {k + "class_mean": _mean(class_loss), k + "class_std": _std(class_loss),
            k + "bbox_mean": _mean(bbox_loss), k + "bbox_std": _std(bbox_loss),
            k + "mean_coord_error": _mean(errors), k + "detection_score": _mean(scores),
            "detection_at": {key: float(np.mean(v)) for key, v in det_at.items()}}
