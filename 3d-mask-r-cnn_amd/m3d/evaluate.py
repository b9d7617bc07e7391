"""Detection unmolding and mask-IoU evaluation on libm3d (csrc/unmold.hip): the
reference's MRCNN_EVALUATION chain predict -> unmold_detections
(core/models.py:7198-7419) -> compute_overlaps_masks (core/utils.py:312-334) ->
compute_matches / compute_ap (core/utils.py:1160-1248) for one image.

``unmold_detections`` turns MaskRCNN.detect's detections [max_inst,8] and
box-local mrcnn_mask [max_inst,m,m,m,C] probabilities into instance masks of the
volume; ``mask_overlaps`` scores them against ground-truth masks [H,W,D,G]
(uint8, G innermost) without building the reference's [H,W,D,N] masks: one pass
over each detection's box voxels counts the intersections as integers.
``compute_matches`` / ``compute_ap`` are the reference's greedy matching and
VOC-style AP in numpy on the [N,G] IoU matrix -- the end of the pipeline, after
one copy to the host.  With ``labels=True`` the chain also builds the
segmentation volume of instance labels on the device (``Unmolded.labels``,
``label_stack`` for the TIFF page order), its pixelwise tp / fp / fn against
the ground truth (``pixelwise_counts``), and the reference's pixelwise,
instance-Dice and mask-level detection metrics (core/models.py:6153-6282,
6644-6721) on the host from the integer counts.  GPU only: there is no CPU
fallback.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, ops

OK, NOT_KEPT, RANGE, FLAT, FAINT, EMPTY, SPARSE = range(7)
STATUS_NAMES = ("OK", "NOT_KEPT", "RANGE", "FLAT", "FAINT", "EMPTY", "SPARSE")
STAT_NAMES = ("min", "max", "mean", "std", "p50", "p95", "thr", "resize_thr")
MAX_GRID = 32768            # m^3 at most (the grid is sorted in LDS)


class Unmolded:
    """Device tensors of one image's unmolded detections:

      small     [max_inst, m^3] uint8   thresholded + cleaned box-local grids
      box_i     [max_inst, 6] int32     (y1,x1,z1,y2,x2,z2), clipped to the volume
      status    [max_inst] int32        OK / NOT_KEPT / RANGE / FLAT / FAINT / EMPTY / SPARSE
      stats     [max_inst, 8] float64   STAT_NAMES
      area_pred [max_inst] int32        set voxels of each instance mask
      dense     [max_inst,H,W,D] uint8  (dense=True)   masks = its [H,W,D,max_inst] view
      seg_union [H,W,D] uint8           (union=True)
      labels    [H,W,D] int32           (labels=True)  the instance label volume
      label_of  [max_inst] int32        (labels=True)  each row's label, 0 = not listed

    A detection whose status is not OK has an all-zero mask, as in the reference."""

    def __init__(self, detections, image_shape, m, small, box_i, status, stats, area_pred, dense, seg_union):
        self.detections, self.image_shape, self.m = detections, tuple(image_shape), m
        self.small, self.box_i, self.status, self.stats, self.area_pred = small, box_i, status, stats, area_pred
        self.dense, self.seg_union = dense, seg_union
        self.overlaps = None        # (iou, inter, area_pred, area_gt) when unmold_detections got gt_masks
        self.labels = self.label_of = None

    @property
    def masks(self):
        return None if self.dense is None else self.dense.permute(1, 2, 3, 0)

    def compact(self):
        """One synchronising copy of the small tensors -> dict of numpy arrays
        for the kept detections, in detection order (the reference's list:
        class id > 0 and every box extent > 0.5 voxel): ``boxes`` [K,6] float32
        pixels, ``scores``, ``class_ids``, ``rows`` (their detection rows),
        ``status``, ``area``.  Raises if any status is RANGE (logits were
        passed: the sigmoid branch is not built)."""
        return self._to_host()

    def label_stack(self):
        """The label volume in TIFF page order: device tensor [D,H,W], uint8 when
        max_inst <= 255 (every label fits), else uint16 -- chosen from the
        shape, so nothing synchronises."""
        if self.labels is None:
            raise ValueError("label_stack needs unmold_detections(..., labels=True)")
        H, W, D = self.image_shape
        wide = int(self.status.shape[0]) > 255
        out = torch.empty((D, H, W), device=self.labels.device, dtype=torch.uint16 if wide else torch.uint8)
        _lib.check(_lib.load().m3d_labels_stack(_lib.ptr(self.labels), H, W, D, 2 if wide else 1, _lib.ptr(out),
                                                _lib.stream()), "m3d_labels_stack")
        return out

    def _to_host(self, iou=None, inter=None, area_gt=None, gt_ids=None, label_of=None):
        """compact(), with the [max_inst,G] overlaps, area_gt [G] and device-side
        GT class ids [G] riding the same single copy (one int32 matrix: a row
        per detection, one more for the two per-GT vectors).  With ``label_of``
        [max_inst] (one more column of that copy) the list is the listed rows
        (label_of > 0: the keep filter applied) and ``label_of`` is returned."""
        n = self.detections.shape[0]
        cols = [self.detections.view(torch.int32), self.status[:, None], self.area_pred[:, None]]
        G = 0 if inter is None else int(inter.shape[1])
        if G:
            cols += [inter, iou.view(torch.int32)]
        if label_of is not None:
            cols.append(label_of[:, None])
        packed = torch.cat(cols, 1)
        if G:
            last = torch.zeros((1, packed.shape[1]), dtype=torch.int32, device=packed.device)
            last[0, 10:10 + G] = area_gt
            if gt_ids is not None:
                last[0, 10 + G:10 + 2 * G] = gt_ids.to(torch.int32)
            packed = torch.cat([packed, last], 0)
        host = packed.cpu().numpy()
        det = host[:n, :8].copy().view(np.float32).reshape(n, 8)
        status, area = host[:n, 8], host[:n, 9]
        if (status == RANGE).any():
            raise ValueError("unmold_detections: mrcnn_mask holds values outside [-0.1, 1.1] (logits?) in rows "
                             f"{np.flatnonzero(status == RANGE).tolist()}; pass probabilities")
        rows = np.flatnonzero(status != NOT_KEPT if label_of is None else host[:n, -1] > 0)
        H, W, D = self.image_shape
        boxes = det[rows, :6] * np.array([H, W, D, H, W, D], np.float32)
        out = {"boxes": boxes, "scores": det[rows, 7], "class_ids": det[rows, 6].astype(np.int32), "rows": rows,
               "status": status[rows].copy(), "area": area[rows].copy()}
        if G:
            out["inter"] = host[:n, 10:10 + G][rows].copy()
            out["iou"] = host[:n, 10 + G:10 + 2 * G].copy().view(np.float32).reshape(n, G)[rows]
            out["area_gt"] = host[n, 10:10 + G].copy()
            out["gt_ids"] = host[n, 10 + G:10 + 2 * G].copy()
        if label_of is not None:
            out["label_of"] = host[:n, -1].copy()
        return out


def _shape3(image_shape):
    s = tuple(int(v) for v in image_shape)[:3]
    if len(s) != 3:
        raise ValueError("image_shape must be (H, W, D)")
    return s


def _gt_u8(gt):
    if gt.dtype == torch.bool:
        gt = gt.view(torch.uint8) if gt.is_contiguous() else gt.to(torch.uint8)
    elif gt.dtype != torch.uint8:
        gt = (gt != 0).to(torch.uint8)
    return gt.contiguous()


def _check_gt(gt_masks, shape):
    ops._dev(gt_masks)
    if gt_masks.dim() == 5 and gt_masks.shape[0] == 1:
        gt_masks = gt_masks[0]
    if gt_masks.dim() != 4 or tuple(gt_masks.shape[:3]) != tuple(shape):
        raise ValueError(f"gt_masks must be [H,W,D,G] with (H,W,D) = {tuple(shape)}, got {tuple(gt_masks.shape)}")
    return _gt_u8(gt_masks)


def _count(u, gt):
    """The one traversal of every box: area_pred, and with gt [H,W,D,G] also
    inter, area_gt and the IoU, then the after-resize rejection.  Returns
    (iou, inter, area_pred, area_gt); the first, second and last are None
    without gt."""
    H, W, D = u.image_shape
    n = int(u.status.shape[0])
    G = 0 if gt is None else int(gt.shape[3])
    dev = u.status.device
    L, p, s = _lib.load(), _lib.ptr, _lib.stream()
    area = torch.empty(n, device=dev, dtype=torch.int32)
    inter = area_gt = iou = None
    if gt is not None:
        inter = torch.empty((n, G), device=dev, dtype=torch.int32)
        area_gt = torch.empty(G, device=dev, dtype=torch.int32)
        iou = torch.empty((n, G), device=dev, dtype=torch.float32)
    _lib.check(L.m3d_unmold_overlaps(p(u.small), p(u.box_i), p(u.status), p(u.stats), n, u.m, H, W, D,
                                     p(gt) if G else None, G, p(area), p(inter) if G else None, s),
               "m3d_unmold_overlaps")
    if G:
        _lib.check(L.m3d_mask_areas(p(gt), H, W, D, G, p(area_gt), s), "m3d_mask_areas")
    _lib.check(L.m3d_unmold_finalize(p(u.box_i), p(u.status), n, G, p(area), p(inter) if G else None,
                                     p(area_gt) if G else None, p(iou) if G else None, s), "m3d_unmold_finalize")
    return iou, inter, area, area_gt


def _keep_u8(keep, n):
    ops._dev(keep)
    if keep.dtype not in (torch.bool, torch.uint8) or tuple(keep.shape) != (n,):
        raise ValueError(f"keep must be a bool / uint8 tensor [{n}], got {keep.dtype} {tuple(keep.shape)}")
    keep = keep.contiguous()
    return keep.view(torch.uint8) if keep.dtype == torch.bool else keep


def unmold_detections(detections, mrcnn_mask, image_shape, dense=False, union=False, gt_masks=None, labels=False,
                      keep=None):
    """detections [max_inst,8], mrcnn_mask [max_inst,m,m,m,C] probabilities of
    one image (a leading batch axis of 1 is accepted) -> Unmolded.  With
    ``gt_masks`` [H,W,D,G] the overlaps are counted in the same traversal of
    the boxes and left in ``.overlaps`` (what mask_overlaps returns).  With
    ``labels`` the instance label volume ``.labels`` [H,W,D] int32 and the
    rows' labels ``.label_of`` are built (the reference's seg[full > 0.5] = j
    + 1 over its kept list, core/models.py:7023-7069); ``keep`` (bool / uint8
    device tensor [max_inst]) drops rows from that list -- the caller's
    confidence / size / NMS filters.  Nothing synchronises."""
    ops._dev(detections, mrcnn_mask)
    if detections.dim() == 3 and detections.shape[0] == 1:
        detections = detections[0]
    if mrcnn_mask.dim() == 6 and mrcnn_mask.shape[0] == 1:
        mrcnn_mask = mrcnn_mask[0]
    if detections.dim() != 2 or detections.shape[1] != 8:
        raise ValueError(f"detections must be [max_inst,8], got {tuple(detections.shape)}")
    n = int(detections.shape[0])
    if keep is not None:
        if not labels:
            raise ValueError("keep filters the label list: pass labels=True")
        keep = _keep_u8(keep, n)
    if mrcnn_mask.dim() != 5 or mrcnn_mask.shape[0] != n or len(set(mrcnn_mask.shape[1:4])) != 1:
        raise ValueError(f"mrcnn_mask must be [max_inst,m,m,m,C], got {tuple(mrcnn_mask.shape)}")
    m, C = int(mrcnn_mask.shape[1]), int(mrcnn_mask.shape[4])
    H, W, D = _shape3(image_shape)
    gt = None if gt_masks is None else _check_gt(gt_masks, (H, W, D))
    det, mask = ops._c(detections.detach()), ops._c(mrcnn_mask.detach())
    dev = det.device
    L, p, s = _lib.load(), _lib.ptr, _lib.stream()
    small = torch.empty((n, m ** 3), device=dev, dtype=torch.uint8)
    box_i = torch.empty((n, 6), device=dev, dtype=torch.int32)
    status = torch.empty(n, device=dev, dtype=torch.int32)
    stats = torch.empty((n, 8), device=dev, dtype=torch.float64)
    _lib.check(L.m3d_unmold_prepare(p(det), p(mask), n, m, C, H, W, D, p(small), p(box_i), p(status), p(stats), s),
               "m3d_unmold_prepare")
    u = Unmolded(det, (H, W, D), m, small, box_i, status, stats, None, None, None)
    counted = _count(u, gt)
    u.area_pred = counted[2]
    if gt is not None:
        u.overlaps = counted
    if dense:
        u.dense = torch.zeros((n, H, W, D), device=dev, dtype=torch.uint8)
    if union:
        u.seg_union = torch.zeros((H, W, D), device=dev, dtype=torch.uint8)
    if dense or union:
        _lib.check(L.m3d_unmold_paste(p(small), p(box_i), p(status), p(stats), n, m, H, W, D, p(u.dense),
                                      p(u.seg_union), s), "m3d_unmold_paste")
    if labels:
        u.label_of = torch.empty(n, device=dev, dtype=torch.int32)
        u.labels = torch.empty((H, W, D), device=dev, dtype=torch.int32)
        _lib.check(L.m3d_unmold_labels(p(small), p(box_i), p(status), p(stats), p(keep), n, m, H, W, D,
                                       p(u.label_of), p(u.labels), s), "m3d_unmold_labels")
    return u


def pixelwise_counts(labels, gt_masks):
    """labels [H,W,D] int32, gt_masks [H,W,D,G] (uint8 / bool, set = non-zero; G
    may be 0) -> device int64 [3]: tp, fp, fn of (labels > 0) against (any GT
    mask set), one streaming pass.  Nothing synchronises."""
    ops._dev(labels)
    if labels.dim() != 3 or labels.dtype != torch.int32:
        raise ValueError(f"labels must be int32 [H,W,D], got {labels.dtype} {tuple(labels.shape)}")
    H, W, D = (int(v) for v in labels.shape)
    gt = _check_gt(gt_masks, (H, W, D))
    G = int(gt.shape[3])
    out = torch.empty(3, device=labels.device, dtype=torch.int64)
    _lib.check(_lib.load().m3d_label_pixelwise(_lib.ptr(labels.contiguous()), _lib.ptr(gt) if G else None, H, W, D,
                                               G, _lib.ptr(out), _lib.stream()), "m3d_label_pixelwise")
    return out


def mask_areas(gt_masks):
    """[H,W,D,G] uint8 -> area_gt [G] int32 (set = non-zero)."""
    ops._dev(gt_masks)
    if gt_masks.dim() != 4:
        raise ValueError("gt_masks must be [H,W,D,G]")
    gt = _gt_u8(gt_masks)
    H, W, D, G = (int(v) for v in gt.shape)
    out = torch.zeros(G, device=gt.device, dtype=torch.int32)
    _lib.check(_lib.load().m3d_mask_areas(_lib.ptr(gt), H, W, D, G, _lib.ptr(out), _lib.stream()), "m3d_mask_areas")
    return out


def mask_overlaps(unmolded, gt_masks):
    """(iou float32 [max_inst,G], inter int32 [max_inst,G], area_pred int32
    [max_inst], area_gt int32 [G]) of already unmolded masks against gt_masks
    [H,W,D,G] (uint8 / bool, set = non-zero).  iou = inter / (area_pred +
    area_gt - inter) in float32; 0 / 0 is NaN, as in numpy.  This walks the
    boxes again; when the GT masks are known up front, pass them to
    unmold_detections instead.  Nothing synchronises."""
    return _count(unmolded, _check_gt(gt_masks, unmolded.image_shape))


def _preference(row):
    """GT indices in the order one prediction tries them: an undefined IoU (NaN:
    empty against empty) ranks above every number, then larger IoU first, the
    later GT first among equals -- the order of a reversed stable ascending
    sort, which is what the reference's matching walks."""
    rank = np.where(np.isnan(row), np.inf, row)
    return np.lexsort((np.arange(len(row)), rank))[::-1]


def compute_matches(overlaps, pred_class_ids, gt_class_ids, iou_threshold=0.5, score_threshold=0.0):
    """Greedy one-to-one assignment of predictions (in the given order: detection
    order is descending score) to ground truths on the host [N,G] IoU matrix,
    the rule of the reference's compute_matches (core/utils.py:1160-1206) ->
    (gt_match [G] int, pred_match [N] int, matched IoUs); -1 = unmatched.

    A prediction looks at the GTs in _preference order, cut where the IoU first
    drops under ``score_threshold``.  GTs already assigned are passed over.  At
    the first free GT under ``iou_threshold`` it gives up; before that, the
    first free GT of its own class is its match (one of another class is
    passed over too).  A NaN IoU is under neither threshold, as there."""
    iou = np.asarray(overlaps)
    n_pred, n_gt = iou.shape
    pred_cls, gt_cls = np.asarray(pred_class_ids), np.asarray(gt_class_ids)
    taken = np.zeros(n_gt, bool)
    pred_match = np.full(n_pred, -1, np.int64)
    gt_match = np.full(n_gt, -1, np.int64)
    matched = []
    for i in range(n_pred):
        cand = _preference(iou[i])
        under_score = np.flatnonzero(iou[i, cand] < score_threshold)
        if under_score.size:
            cand = cand[:under_score[0]]
        cand = cand[~taken[cand]]
        under_iou = np.flatnonzero(iou[i, cand] < iou_threshold)
        if under_iou.size:
            cand = cand[:under_iou[0]]
        cand = cand[gt_cls[cand] == pred_cls[i]]
        if cand.size:
            j = int(cand[0])
            taken[j] = True
            gt_match[j], pred_match[i] = i, j
            matched.append(iou[i, j])
    return gt_match, pred_match, matched


def compute_ap(overlaps, pred_class_ids, gt_class_ids, iou_threshold=0.5):
    """VOC-style average precision at one IoU threshold, the measure of the
    reference's compute_ap (core/utils.py:1209-1248) -> (mAP, precision,
    recall, matched IoUs).

    After each prediction k: precision_k = hits / (k + 1), recall_k = hits / G
    (rounded to float32 as there).  The curve gets the end points (recall 0,
    precision 0) and (recall 1, precision 0), precision becomes its running
    maximum from the right, and mAP sums precision times the recall step over
    the points where recall moves.  precision / recall are the final ratios."""
    gt_match, pred_match, matched = compute_matches(overlaps, pred_class_ids, gt_class_ids, iou_threshold)
    n_pred, n_gt = len(pred_match), len(gt_match)
    hits = np.cumsum(pred_match >= 0)
    total = int(hits[-1]) if n_pred else 0
    with np.errstate(divide="ignore", invalid="ignore"):
        prec = np.zeros(n_pred + 2)
        rec = np.zeros(n_pred + 2)
        prec[1:-1] = hits / np.arange(1, n_pred + 1)
        rec[1:-1] = hits.astype(np.float32) / np.float32(n_gt)
        rec[-1] = 1.0
        envelope = np.maximum.accumulate(prec[::-1])[::-1]
        step = np.diff(rec)
        moves = step != 0
        mAP = 0.0
        for term in (step[moves] * envelope[1:][moves]).tolist():   # left to right: one defined order
            mAP += term
        precision = float(np.float64(total) / np.float64(n_pred))
        recall = float(np.float64(total) / np.float64(n_gt))
    return mAP, precision, recall, matched


def pixelwise_metrics(tp, fp, fn):
    """(precision, recall, f1, iou) of the reference's _pixelwise_metrics
    (core/models.py:6153-6164) from its three int64 counts: float64, its 1e-9
    terms and its zero-denominator branches."""
    tp, fp, fn = np.int64(tp), np.int64(fp), np.int64(fn)
    prec = (tp / (tp + fp + 1e-9)) if (tp + fp) > 0 else 0.0
    rec = (tp / (tp + fn + 1e-9)) if (tp + fn) > 0 else 0.0
    f1 = (2.0 * prec * rec / (prec + rec + 1e-9)) if (prec + rec) > 0 else 0.0
    iou = (tp / (tp + fp + fn + 1e-9)) if (tp + fp + fn) > 0 else 0.0
    return float(prec), float(rec), float(f1), float(iou)


def _mask_iou(inter, area_pred, area_gt):
    inter = np.asarray(inter).astype(np.int64)
    p_sum, t_sum = np.asarray(area_pred).astype(np.int64), np.asarray(area_gt).astype(np.int64)
    union = (p_sum[:, None] + t_sum[None, :]) - inter
    return inter, p_sum, t_sum, inter / np.maximum(union, 1)


def instance_dice(inter, area_pred, area_gt, iou_thr=0.5):
    """The reference's _instance_dice (core/models.py:6166-6282) on the integer
    counts inter [K,G], area_pred [K], area_gt [G] of the listed masks ->
    (mean, std, n).  iou = inter / max(union, 1) in float64; repeatedly the
    global argmax over the unused rows and columns, until it is under
    ``iou_thr``; Dice = 2 inter / (P + T) of each pair; np.mean / np.std."""
    inter, p_sum, t_sum, iou = _mask_iou(inter, area_pred, area_gt)
    K, G = iou.shape
    if K == 0 or G == 0:
        return 0.0, 0.0, 0
    used_p, used_g = np.zeros(K, bool), np.zeros(G, bool)
    dices = []
    while True:
        masked = iou.copy()
        masked[used_p, :] = -1.0
        masked[:, used_g] = -1.0
        k, g = np.unravel_index(np.argmax(masked), masked.shape)
        if masked[k, g] < iou_thr:
            break
        denom = p_sum[k] + t_sum[g]
        dices.append(float((2.0 * inter[k, g] / denom) if denom > 0 else 0.0))
        used_p[k] = used_g[g] = True
    if not dices:
        return 0.0, 0.0, 0
    return float(np.mean(dices)), float(np.std(dices)), len(dices)


def detection_performance(inter, area_pred, area_gt, thr=0.5):
    """The mask-level detection counts of the reference's _compute_mask_metrics
    (core/models.py:6663-6706) on the same counts -> dict tp, fp, fn, recall,
    precision: the best remaining pair is matched and its row and column are
    zeroed, until the best IoU is under ``thr``.  Without predictions or
    without ground truths (where the reference reports nothing) every
    prediction is a fp and every ground truth a fn."""
    _, _, _, iou = _mask_iou(inter, area_pred, area_gt)
    K, G = iou.shape
    matched_p, matched_g = np.zeros(K, bool), np.zeros(G, bool)
    while K > 0 and G > 0:
        i, j = np.unravel_index(np.argmax(iou), iou.shape)
        if iou[i, j] < thr:
            break
        matched_p[i] = matched_g[j] = True
        iou[i, :] = 0
        iou[:, j] = 0
    tp = np.sum(matched_p)
    fp = K - tp
    fn = G - np.sum(matched_g)
    return {"tp": int(tp), "fp": int(fp), "fn": int(fn), "recall": float(tp / (tp + fn)) if (tp + fn) > 0 else 0.0,
            "precision": float(tp / (tp + fp)) if (tp + fp) > 0 else 0.0}


def write_detection_csv(path, class_ids, boxes):
    """The reference's save_classes_and_boxes table (core/models.py:6313-6336):
    header class,y1,x1,z1,y2,x2,z2, then one line per listed detection in label
    order; boxes [K,6] float32 pixels as in compact()["boxes"], written in
    their shortest text that reads back to the same float32."""
    import csv
    with open(path, "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(["class", "y1", "x1", "z1", "y2", "x2", "z2"])
        for cid, box in zip(class_ids, np.asarray(boxes, np.float32)):
            w.writerow([int(cid)] + [str(v) for v in box])


def evaluate_detections(detections, mrcnn_mask, image_shape, gt_class_ids, gt_masks, iou_threshold=0.5, labels=False,
                        keep=None):
    """unmold + overlaps (one traversal of the boxes) -> AP for one image ->
    dict: mAP, precision, recall, ious (matched), iou / inter [K,G] of the kept
    detections (host), boxes, scores, class_ids, rows, status, area_pred,
    area_gt, and the device-side ``unmolded``.  Every result reaches the host
    in one synchronising copy; raises on status RANGE.

    With ``labels`` also: ``labels`` (the device label volume [H,W,D] int32),
    ``label_of`` (host, [max_inst]), ``pixelwise`` (precision, recall, f1, iou)
    with its ``pixelwise_counts`` (tp, fp, fn), ``instance_dice`` (mean, std,
    n) and ``detection_performance``.  ``keep`` (needs labels) restricts
    ``rows`` and every per-row result, the AP included, to the listed rows.
    label_of rides the packed copy as one more column; the three pixelwise
    counts take one more 24-byte copy."""
    u = unmold_detections(detections, mrcnn_mask, image_shape, gt_masks=gt_masks, labels=labels, keep=keep)
    iou, inter, _, area_gt = u.overlaps
    G = int(inter.shape[1])
    on_dev = torch.is_tensor(gt_class_ids) and gt_class_ids.is_cuda
    if on_dev and gt_class_ids.numel() != G:
        raise ValueError(f"gt_class_ids has {gt_class_ids.numel()} entries for {G} GT masks")
    counts = pixelwise_counts(u.labels, gt_masks) if labels else None
    if G:
        k = u._to_host(iou, inter, area_gt, gt_class_ids.reshape(-1) if on_dev else None, label_of=u.label_of)
    else:
        k = u._to_host(label_of=u.label_of)
        k.update(inter=np.zeros((len(k["rows"]), 0), np.int32), iou=np.zeros((len(k["rows"]), 0), np.float32),
                 area_gt=np.zeros(0, np.int32), gt_ids=np.zeros(0, np.int32))
    if on_dev:
        gt_ids = k["gt_ids"]
    else:
        gt_ids = np.asarray(gt_class_ids.numpy() if torch.is_tensor(gt_class_ids) else gt_class_ids)
        gt_ids = gt_ids.reshape(-1).astype(np.int32)
        if len(gt_ids) != G:
            raise ValueError(f"gt_class_ids has {len(gt_ids)} entries for {G} GT masks")
    mAP, precision, recall, ious = compute_ap(k["iou"], k["class_ids"], gt_ids, iou_threshold)
    out = {"mAP": mAP, "precision": precision, "recall": recall, "ious": ious, "iou": k["iou"], "inter": k["inter"],
           "boxes": k["boxes"], "scores": k["scores"], "class_ids": k["class_ids"], "rows": k["rows"],
           "status": k["status"], "area_pred": k["area"], "area_gt": k["area_gt"], "unmolded": u}
    if labels:
        tp, fp, fn = (int(v) for v in counts.cpu().numpy())
        out.update(labels=u.labels, label_of=k["label_of"], pixelwise_counts=(tp, fp, fn),
                   pixelwise=pixelwise_metrics(tp, fp, fn),
                   instance_dice=instance_dice(k["inter"], k["area"], k["area_gt"]),
                   detection_performance=detection_performance(k["inter"], k["area"], k["area_gt"]))
    return out
