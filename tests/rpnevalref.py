"""NumPy restatement of the per-image scoring of the reference's rpn_evaluation
(core/utils.py:1289-1392, with compute_overlaps_3d 78-144 and denorm_boxes
1562-1574): what m3d_rpn_eval_proposals computes, in the reference's order of
operations.  Every value is float32 and every operation a single float32
NumPy ufunc, so nothing is contracted; the two threshold compares are written
with their precision spelled out (the reference leaves them to the installed
NumPy's scalar promotion):

    match   np.float64(iou) > thr         (a float32 scalar against a Python float)
    grid    iou >= np.float32(thr)        (a float32 array against a scalar)
"""
import numpy as np

NONE = np.int32(2 ** 31 - 1)


def pixel_boxes(rois, shape):
    """rois [R,6] normalised -> (clamped pixel boxes [R,6] float32, valid [R] bool)."""
    H, W, D = (int(v) for v in shape)
    px = (np.asarray(rois, np.float32).reshape(-1, 6) * np.array([H, W, D, H, W, D], np.float32)).astype(np.float32)
    lo = np.array([0, 0, 0, 1, 1, 1], np.float32)
    hi = np.array([H, W, D, H, W, D], np.float32)
    with np.errstate(invalid="ignore"):
        px = np.minimum(np.maximum(px, lo), hi)                 # np.clip: NaN stays NaN
        valid = (px[:, 3] > px[:, 0]) & (px[:, 4] > px[:, 1]) & (px[:, 5] > px[:, 2])
    return px, valid


def _corners(b):
    b = np.asarray(b, np.float32).reshape(-1, 6)
    return np.concatenate([np.minimum(b[:, :3], b[:, 3:]), np.maximum(b[:, :3], b[:, 3:])], 1)


def overlaps(gt, boxes):
    """[G,6] x [N,6] pixel boxes -> IoU [G,N] float32 (compute_overlaps_3d)."""
    a, b = _corners(gt)[:, None, :], _corners(boxes)[None, :, :]
    zero, one = np.float32(0), np.float32(1)
    h = np.maximum(np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 0], b[..., 0]), zero)
    w = np.maximum(np.minimum(a[..., 4], b[..., 4]) - np.maximum(a[..., 1], b[..., 1]), zero)
    d = np.maximum(np.minimum(a[..., 5], b[..., 5]) - np.maximum(a[..., 2], b[..., 2]), zero)
    inter = (h * w) * d
    va = ((a[..., 3] - a[..., 0]) * (a[..., 4] - a[..., 1])) * (a[..., 5] - a[..., 2])
    vb = ((b[..., 3] - b[..., 0]) * (b[..., 4] - b[..., 1])) * (b[..., 5] - b[..., 2])
    union = np.maximum((va + vb) - inter, np.float32(1e-10))
    out = np.minimum(np.maximum(inter / union, zero), one)
    assert out.dtype == np.float32
    return out


def score(rois, gt, shape, topk, match_iou, iou_grid):
    """One image -> dict: ``assoc`` [G] int32, ``matched`` [G,6] float32,
    ``first_hit`` [T,G] int32, ``counts`` [2] int32, ``iou`` [G,R] float32 (0
    in the columns of invalid rows)."""
    rois = np.asarray(rois, np.float32).reshape(-1, 6)
    gt = np.asarray(gt, np.float32).reshape(-1, 6)
    R, G, T = len(rois), len(gt), len(iou_grid)
    px, valid = pixel_boxes(rois, shape)
    rows = np.flatnonzero(valid)
    iou = np.zeros((G, R), np.float32)
    iou[:, rows] = overlaps(gt, px[rows])
    kmatch = min(int(topk), R)
    assoc = np.full(G, -1, np.int32)
    for j in rows[rows < kmatch]:                      # the reference's walk over its compacted list, in row order
        g = int(np.argmax(iou[:, j]))
        if assoc[g] == -1 and np.float64(iou[g, j]) > float(match_iou):
            assoc[g] = j
    matched = np.zeros((G, 6), np.float32)
    matched[assoc >= 0] = px[assoc[assoc >= 0]]
    first_hit = np.full((T, G), NONE, np.int32)
    for t, thr in enumerate(iou_grid):
        hit = (iou >= np.float32(thr)) & valid[None, :]
        any_hit = hit.any(axis=1)
        if any_hit.any():
            first_hit[t, any_hit] = np.argmax(hit[any_hit], axis=1)
    counts = np.array([int(valid[:kmatch].sum()), rows[0] if len(rows) else NONE], np.int32)
    return {"assoc": assoc, "matched": matched, "first_hit": first_hit, "counts": counts, "iou": iou}
