"""Training augmentations (core/data_generators.py:13-167).

``apply_minimal_augs_3d(image, boxes, masks, config, rng)`` is the reference's
function of the same name with the image and the masks on the device: the
flip decisions are drawn on the host from ``rng`` in the reference's order
(``rng.rand() < AUG_PROB`` for Y, then X, then Z, a draw only for an enabled
axis), the flips, the brightness leg and the Gaussian leg run in
``m3d_augment_image`` / ``m3d_flip_masks_u8`` / ``m3d_flip_boxes``.  The noise
comes from Philox4x32-10 keyed by two further 32-bit draws from ``rng`` (made
only when a noise leg is on): the reference draws from an unseeded
``np.random.RandomState(None)``, whose stream cannot be reproduced, so the
formula and the distribution are matched and a run is reproducible from the
seed of ``rng``.

``jitter_boxes_3d`` is host numpy (tens of boxes) with the reference's draw
order, clipping, IoU filter and top-``max_keep`` selection, drawing from the
``rng`` passed in instead of the global ``np.random``.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, ops
from ._lib import check, ptr, stream

FLIP_Y, FLIP_X, FLIP_Z = 1, 2, 4


def draw_flips(config, rng) -> int:
    """The flip mask of one call: a draw per enabled axis, Y, X, Z."""
    p = float(getattr(config, "AUG_PROB", 0.5))
    mask = 0
    if bool(getattr(config, "AUG_FLIP_Y", True)) and rng.rand() < p:
        mask |= FLIP_Y
    if bool(getattr(config, "AUG_FLIP_X", True)) and rng.rand() < p:
        mask |= FLIP_X
    if bool(getattr(config, "AUG_FLIP_Z", False)) and rng.rand() < p:
        mask |= FLIP_Z
    return mask


def flip_boxes(boxes, shape, mask):
    """[N,6] pixel boxes (y1,x1,z1,y2,x2,z2) with exclusive ends under the
    flips of ``mask`` in a volume of ``shape`` = (Y, X, Z): y1' = Y - y2, y2'
    = Y - y1 and likewise for x and z, in float32.  A numpy array is flipped on
    the host, a device tensor by ``m3d_flip_boxes``."""
    Y, X, Z = (int(v) for v in shape[:3])
    if torch.is_tensor(boxes):
        ops._dev(boxes)
        b = boxes.detach().to(torch.float32).reshape(-1, 6).contiguous()
        out = torch.empty_like(b)
        check(_lib.load().m3d_flip_boxes(ptr(b), int(b.shape[0]), Y, X, Z, int(mask), ptr(out), stream()),
              "flip_boxes")
        return out
    b = np.asarray(boxes, np.float32).reshape(-1, 6).copy()
    for axis, ext in enumerate((Y, X, Z)):
        if mask & (1 << axis) and b.size:
            lo = np.float32(ext) - b[:, axis + 3]
            hi = np.float32(ext) - b[:, axis]
            b[:, axis], b[:, axis + 3] = lo, hi
    return b


def augment_image(image, flip_mask=0, brightness_delta=0.0, noise_std=0.0, seed=(0, 0)):
    """``m3d_augment_image`` on a device [H,W,D] (or [H,W,D,1]) float32 image,
    out of place; seed = (lo, hi) 32-bit words of the Philox key."""
    ops._dev(image)
    x = image.detach().to(torch.float32).contiguous()
    H, W, D = (int(v) for v in x.shape[:3])
    if x.numel() != H * W * D:
        raise ValueError(f"augment_image takes [H,W,D] or [H,W,D,1], got {tuple(image.shape)}")
    L = _lib.load()
    out = torch.empty_like(x)
    bd = float(brightness_delta)
    wsb = int(L.m3d_augment_image_workspace_bytes(H, W, D)) if bd > 0 else 0
    ws = torch.empty(max(wsb, 4), dtype=torch.uint8, device=x.device) if wsb else None
    check(L.m3d_augment_image(ptr(x), H, W, D, int(flip_mask), bd, float(noise_std), int(seed[0]) & 0xFFFFFFFF,
                              int(seed[1]) & 0xFFFFFFFF, ptr(out), ptr(ws), wsb, stream()), "augment_image")
    return out


def flip_masks(masks, flip_mask):
    """``m3d_flip_masks_u8`` on device [H,W,D,G] uint8 / bool masks, out of place."""
    ops._dev(masks)
    if masks.dim() != 4:
        raise ValueError(f"flip_masks takes [H,W,D,G], got {tuple(masks.shape)}")
    kind = masks.dtype
    m = masks.contiguous()
    m = m.view(torch.uint8) if kind == torch.bool else m.to(torch.uint8)
    H, W, D, G = (int(v) for v in m.shape)
    if G == 0 or not flip_mask:
        return masks.clone()
    out = torch.empty_like(m)
    check(_lib.load().m3d_flip_masks_u8(ptr(m), H, W, D, G, int(flip_mask), ptr(out), stream()), "flip_masks_u8")
    return out.view(torch.bool) if kind == torch.bool else out


def apply_minimal_augs_3d(image, boxes, masks, config, rng):
    """-> (image, boxes, masks) as the reference's apply_minimal_augs_3d
    (core/data_generators.py:13-86).  image: device [H,W,D] or [H,W,D,1]
    float32; boxes: [N,6] pixel boxes, numpy (flipped on the host) or a device
    tensor, or None; masks: device [H,W,D,G] uint8 / bool or None."""
    if image is None:
        return image, boxes, masks
    ops._dev(image)
    mask = draw_flips(config, rng)
    bd = float(getattr(config, "AUG_BRIGHTNESS_DELTA", 0.0))
    ns = float(getattr(config, "AUG_GAUSS_NOISE_STD", 0.0))
    seed = (0, 0)
    if bd > 0 or ns > 0:
        seed = (int(rng.randint(0, 2 ** 32, dtype=np.uint64)), int(rng.randint(0, 2 ** 32, dtype=np.uint64)))
    if mask or bd > 0 or ns > 0:
        image = augment_image(image, mask, max(bd, 0.0), max(ns, 0.0), seed).reshape(image.shape)
    else:
        image = image.clone()
    if boxes is not None:
        boxes = flip_boxes(boxes, image.shape, mask)
    if masks is not None and mask:
        masks = flip_masks(masks, mask)
    return image, boxes, masks


def _iou_with(box, cands):
    """float32 IoU of one box with [K,6] candidates (areas and union floored at 1e-6)."""
    lo = np.maximum(box[:3], cands[:, :3])
    hi = np.minimum(box[3:], cands[:, 3:])
    inter = np.prod(np.maximum(hi - lo, np.float32(0)), axis=1, dtype=np.float32)
    area = np.float32(max(float(np.prod(box[3:] - box[:3], dtype=np.float32)), 1e-6))
    areas = np.maximum(np.prod(cands[:, 3:] - cands[:, :3], axis=1, dtype=np.float32), np.float32(1e-6))
    return inter / np.maximum(area + areas - inter, np.float32(1e-6))


def jitter_boxes_3d(boxes, count=3, scale_sigma=0.10, trans=(2, 2, 1), img_shape=None, iou_thr=0.40, max_keep=None,
                    rng=None):
    """core/data_generators.py:88-167: around every GT box ``count`` candidates
    -- per candidate three ``randn`` scale the extents (1 + sigma r, extents
    floored at one voxel), then three ``randint`` in [-trans, trans] shift the
    centre -- clipped to the image (starts to [0, size - 1], ends to [1, size];
    a candidate clipped to nothing is dropped), kept when their IoU with the
    box is at least ``iou_thr``, the ``max_keep`` best of them when more pass.
    Returns the boxes followed by the kept candidates, box by box, float32.
    The candidate arithmetic is float64 (the reference's, under the numpy its
    pins install), rounded to float32 before the float32 IoU."""
    if boxes is None:
        return boxes
    rng = np.random if rng is None else rng
    gt = np.asarray(boxes, np.float32)
    if gt.size == 0 or count <= 0:
        return gt
    sigma = float(scale_sigma)
    reach = [int(t) for t in trans]
    size = None if img_shape is None else np.asarray(img_shape[:3], np.float64)
    added = []
    for box in gt:
        start, end = box[:3].astype(np.float64), box[3:].astype(np.float64)
        extent = np.maximum(1.0, end - start)
        centre = (start + end) / 2.0
        cands = []
        for _ in range(int(count)):
            scale = np.array([1.0 + rng.randn() * sigma for _ in range(3)])
            shift = np.array([rng.randint(-r, r + 1) for r in reach], np.float64)
            half = np.maximum(1.0, extent * scale) / 2.0
            lo, hi = centre + shift - half, centre + shift + half
            if size is not None:
                lo, hi = np.clip(lo, 0.0, size - 1.0), np.clip(hi, 1.0, size)
                if (hi <= lo).any():
                    continue
            cands.append(np.concatenate([lo, hi]))
        if not cands:
            continue
        cands = np.asarray(cands, np.float32)
        ious = _iou_with(box, cands)
        passed = ious >= np.float32(iou_thr)
        kept = cands[passed]
        if len(kept):
            if isinstance(max_keep, (int, np.integer)) and 0 < max_keep < len(kept):
                kept = kept[np.argsort(ious[passed])[::-1][:int(max_keep)]]
            added.append(kept)
    if not added:
        return gt
    return np.concatenate([gt] + added).astype(np.float32)
