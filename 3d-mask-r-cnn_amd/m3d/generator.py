"""The training generators on the device: ``RPNGenerator`` (below) and the
stored-target ``HeadGenerator`` with its ROI selection (end of the file).

``RPNGenerator(config, dataset, anchors, device)`` joins ``ToyDataset``,
the augmentations, the GT jitter, the target builder and ``RPN.train_step`` the
way the reference's ``RPNGenerator.__getitem__`` / ``data_generator`` does
(core/data_generators.py:933-1012, ``load_image_gt`` 1014-1042): per item

* ``dataset.load_image(id, device=...)``: the raw stack uploaded in its file
  dtype and normalised on the device; ``dataset.load_data`` for the boxes;
* ``apply_minimal_augs_3d`` when ``AUGMENT`` is set and ``MODE == "training"``
  (1038-1042);
* an image without boxes draws another one, up to five times (946-950);
* ``jitter_boxes_3d`` when ``RPN_AUGMENT_GT`` is set, with the ``getattr``
  defaults of 975-983;
* the boxes divided by (H,W,D,H,W,D) and clipped to [0,1], then
  ``RPNTargetBuilder`` (``build_rpn_targets`` at 986).

One image per item, as ``DeviceRPNTargets``: ``IMAGES_PER_GPU > 1`` raises.
Every random choice comes from one ``np.random.RandomState(seed)`` (the
reference uses the unseeded global one), so a seed fixes the whole sequence:
the shuffles, the redraws, the flips, the noise keys, the jitter and the
builder's negative subsampling.

The builder's outputs are reused from item to item: an item's targets are
valid until the next ``__getitem__`` (clone them to keep them).
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .augment import apply_minimal_augs_3d, jitter_boxes_3d
from .targets import RPNTargetBuilder


class RPNGenerator:
    def __init__(self, config, dataset, anchors, device, seed=0, shuffle=True, max_gt=None, list_cap=None):
        if int(getattr(config, "IMAGES_PER_GPU", 1)) > 1:
            raise ValueError("RPNGenerator yields one image per item (DeviceRPNTargets holds one image's targets): "
                             "IMAGES_PER_GPU must be 1")
        self.config = config
        self.dataset = dataset
        self.device = torch.device(device)
        anchors = torch.as_tensor(anchors).reshape(-1, 6).to(self.device)
        ops._dev(anchors)
        self.shape = tuple(int(v) for v in config.IMAGE_SHAPE[:3])
        self.jitter = bool(getattr(config, "RPN_AUGMENT_GT", False))
        self.jitter_args = dict(
            count=int(getattr(config, "RPN_GT_JITTER_PER_BOX", 1)),
            scale_sigma=float(getattr(config, "RPN_GT_JITTER_SCALE_SIGMA", 0.05)),
            trans=tuple(getattr(config, "RPN_GT_JITTER_TRANS", (1, 1, 0))),
            img_shape=self.shape,
            iou_thr=float(getattr(config, "RPN_GT_JITTER_IOU_THR", 0.70)),
            max_keep=int(getattr(config, "RPN_GT_JITTER_MAX_KEEP", 1)))
        if max_gt is None:
            count, keep = max(self.jitter_args["count"], 0), self.jitter_args["max_keep"]
            added = (min(count, keep) if keep > 0 else count) if self.jitter else 0        # jitters kept per box
            max_gt = int(getattr(config, "MAX_GT_INSTANCES", 50)) * (1 + added)
        self.builder = RPNTargetBuilder(anchors, config, max_gt=max_gt, list_cap=list_cap)
        self.augment = bool(getattr(config, "AUGMENT", True)) and getattr(config, "MODE", "training") == "training"
        self.shuffle = bool(shuffle)
        self.rng = np.random.RandomState(seed)
        self.image_ids = np.copy(dataset.image_ids)
        self.last = None
        if self.shuffle:
            self.rng.shuffle(self.image_ids)

    def __len__(self):
        return len(self.image_ids)

    def on_epoch_end(self):
        if self.shuffle:
            self.rng.shuffle(self.image_ids)

    def load_image_gt(self, image_id):
        """(image [H,W,D,1] on the device, pixel boxes [N,6] float32 on the host, class ids)."""
        image = self.dataset.load_image(image_id, device=self.device)
        if tuple(image.shape[:3]) != self.shape:
            raise ValueError(f"image {image_id} is {tuple(image.shape[:3])}, the configuration says {self.shape}: "
                             "the generator does not resize")
        boxes, class_ids, _ = self.dataset.load_data(image_id, masks_needed=False)
        boxes = np.asarray(boxes, np.float32).reshape(-1, 6)
        if self.augment:
            image, boxes, _ = apply_minimal_augs_3d(image, boxes, None, self.config, self.rng)
        return image, boxes, class_ids

    def __getitem__(self, i):
        image_id = int(self.image_ids[i])
        image, boxes, class_ids = self.load_image_gt(image_id)
        tries = 0
        while boxes.size == 0 and tries < 5:
            image_id = int(self.rng.choice(self.image_ids))
            image, boxes, class_ids = self.load_image_gt(image_id)
            tries += 1
        boxes_for_rpn = boxes
        if self.jitter and boxes.size:
            boxes_for_rpn = jitter_boxes_3d(boxes, rng=self.rng, **self.jitter_args)
        H, W, D = self.shape
        gt = np.clip(boxes_for_rpn / np.array([H, W, D, H, W, D], np.float32), 0.0, 1.0).astype(np.float32)
        target_seed = int(self.rng.randint(0, 2 ** 32, dtype=np.uint64))
        targets = self.builder(torch.from_numpy(np.ascontiguousarray(gt)).to(self.device), seed=target_seed)
        self.last = {"image_id": image_id, "boxes": boxes, "boxes_for_rpn": boxes_for_rpn, "gt": gt,
                     "target_seed": target_seed, "tries": tries}
        return image[None], targets


def select_head_rois(target_class_ids, coverage, T, config, rng, training=True):
    """The ROI selection of HeadGenerator.__getitem__ (core/data_generators.py:
    492-640) over the class ids and the mask coverages alone: int64 [T] row
    indices, padded with -1 (``_take_or_pad``'s zero rows).

    ``coverage`` is ``target_mask[i].mean()`` per row, as an array over all
    rows or as a function of the wanted rows, which is called only where the
    reference computes the means (more than T rows, training,
    HEAD_BALANCE_POS, at least one positive).  ``rng`` makes every draw, in
    the reference's call order: the HEAD_SHUFFLE_ROIS shuffle, then either the
    balanced choices (positives, negatives, final shuffle) or the plain choice
    without replacement."""
    tci = np.asarray(target_class_ids).reshape(-1)
    T = int(T)
    total = int(tci.shape[0])
    order = np.arange(total, dtype=np.int32)
    if training and bool(getattr(config, "HEAD_SHUFFLE_ROIS", True)) and total > 0:
        rng.shuffle(order)
    if total <= T:
        sel = order
    elif training and bool(getattr(config, "HEAD_BALANCE_POS", True)):
        all_pos = np.where(tci > 0)[0]
        all_neg = np.where(tci <= 0)[0]
        min_coverage = float(getattr(config, "HEAD_MIN_POSITIVE_COVERAGE", 0.06))
        if len(all_pos) > 0:
            cov = coverage(all_pos) if callable(coverage) else np.asarray(coverage)[all_pos]
            pos_coverages = np.array([float(v) for v in cov])
            strong_mask = pos_coverages >= min_coverage
            strong_pos = all_pos[strong_mask]
            if len(strong_pos) > 0:
                all_pos = strong_pos
            else:                                       # all weak: the best of them
                n_take = min(len(all_pos), max(1, T // 2))
                all_pos = all_pos[np.argsort(pos_coverages)[::-1][:n_take]]
        else:
            all_pos = np.array([], dtype=np.int32)
        empty = np.array([], dtype=np.int32)
        pos_idx = np.intersect1d(order, all_pos) if len(all_pos) > 0 else empty
        neg_idx = np.intersect1d(order, all_neg)
        pos_cnt = int(round(T * float(getattr(config, "HEAD_POS_FRAC", 0.33))))
        if pos_idx.size == 0 and neg_idx.size == 0:
            sel = rng.choice(order, size=min(T, total), replace=False)
        elif pos_idx.size == 0:
            sel = rng.choice(neg_idx, size=T, replace=neg_idx.size < T)
        elif neg_idx.size == 0:
            sel = rng.choice(pos_idx, size=T, replace=pos_idx.size < T)
        else:
            n_pos = min(pos_cnt, pos_idx.size)
            n_neg = T - n_pos
            if n_neg > neg_idx.size:                    # short of negatives: top up with positives
                n_neg = neg_idx.size
                n_pos = T - n_neg
            sel_pos = rng.choice(pos_idx, size=n_pos, replace=pos_idx.size < n_pos)
            sel_neg = rng.choice(neg_idx, size=n_neg, replace=neg_idx.size < n_neg)
            sel = np.concatenate([sel_pos, sel_neg])
            rng.shuffle(sel)
    else:
        sel = rng.choice(order, size=T, replace=False)
    sel = np.asarray(sel, np.int64)
    return np.concatenate([sel, np.full(max(T - sel.size, 0), -1, np.int64)])


class HeadGenerator:
    """The stored-target head generator (core/data_generators.py:180-684) on
    the device: one image per item, read from a prepared ``ToyHeadDataset``.

    Per item: ``dataset.load_packed`` uploads the float16 features and the two
    packed masks as stored; the mask coverages the selection filters on are
    ``m3d_bits_row_counts`` of the packed target mask, count / row_bits in
    float32 (numpy's float32 mean of a 0/1 array); ``select_head_rois`` picks
    TRAIN_ROIS_PER_IMAGE rows on the host; ``m3d.headstore.unpack_gather``
    widens exactly those rows to float32, resized by ``_resize_spatial``'s
    index vectors to MASK_POOL_SIZE / MASK_SHAPE where the stored extent
    differs, padded rows zero.  Returns the reference's six inputs on the
    device: ``[rois_aligned [1,T,P,P,P,C], mask_aligned [1,T,M,M,M,C],
    image_meta [1,16+NUM_CLASSES], target_class_ids [1,T] int32, target_bbox
    [1,T,6], target_mask [1,T,m,m,m]]`` -- the arguments of
    ``MaskRCNN.train_heads_on_features``.  ``last`` holds the item's image id,
    ``sel`` and the gathered ``rois``.

    Differences from the reference, both stated: every draw comes from one
    ``np.random.RandomState(seed)`` (the reference draws from the unseeded
    global one), and the diagnostic prints are not built.  ``training=False``
    disables the ROI shuffle and the balancing, as there."""

    def __init__(self, config, dataset, device, seed=0, shuffle=True, training=True):
        self.config = config
        self.dataset = dataset
        self.device = torch.device(device)
        self.shuffle = bool(shuffle)
        self.training = bool(training)
        self.T = int(getattr(config, "TRAIN_ROIS_PER_IMAGE", 128))
        self.mask_pool = int(getattr(config, "MASK_POOL_SIZE", 14))
        ms = tuple(int(v) for v in config.MASK_SHAPE)
        if len(ms) != 3 or ms != (ms[0],) * 3:
            raise ValueError(f"HeadGenerator: MASK_SHAPE must be a cube, got {ms}")
        self.mask_size = ms[0]
        self.shape = tuple(int(v) for v in config.IMAGE_SHAPE[:3])
        self.num_classes = int(getattr(dataset, "num_classes", getattr(config, "NUM_CLASSES", 2)))
        self.rng = np.random.RandomState(seed)
        self.image_ids = np.copy(dataset.image_ids).astype(np.int64)
        self.last = None
        if self.shuffle:
            self.rng.shuffle(self.image_ids)

    def __len__(self):
        return len(self.image_ids)

    def on_epoch_end(self):
        if self.shuffle:
            self.rng.shuffle(self.image_ids)

    def _coverage(self, packed):
        """rows -> float32 mean of the (resized) target mask of each, from set-bit counts."""
        from . import headstore
        R, m = packed["tm_shape"][0], self.mask_size
        if tuple(packed["tm_shape"][1:4]) == (m, m, m):
            bits = packed["tm_bits"]
        else:       # the reference takes the mean after _resize_spatial: count the resized masks' bits
            bits = headstore.pack_bits(headstore.unpack_gather(packed["tm_bits"], packed["tm_shape"], np.arange(R),
                                                               (m, m, m)))
        counts = headstore.bits_row_counts(bits, R, m ** 3).cpu().numpy()
        cov = counts.astype(np.float32) / np.float32(m ** 3)
        return lambda rows: cov[np.asarray(rows)]

    def __getitem__(self, i):
        from . import headstore
        from .model import compose_image_meta
        image_id = int(self.image_ids[i])
        p = self.dataset.load_packed(image_id, self.device)
        tci = p["target_class_ids"]
        R = int(tci.shape[0])
        ra_shape, ma_shape = tuple(p["rois_aligned"].shape), tuple(p["mask_shape"])
        tm_shape = tuple(p["tm_shape"])
        if len(tm_shape) == 4:
            tm_shape += (1,)
        if len(ma_shape) == 4:
            ma_shape += (1,)
        if len(ra_shape) != 5 or len(ma_shape) != 5 or len(tm_shape) != 5 or tm_shape[4] != 1:
            raise ValueError(f"image {image_id}: stored shapes {ra_shape}, {ma_shape}, {tm_shape} are not "
                             "[T,P,P,P,C], [T,M,M,M,C] and [T,m,m,m(,1)]")
        if not (ra_shape[0] == ma_shape[0] == tm_shape[0] == R == p["rois"].shape[0] == p["target_bbox"].shape[0]):
            raise ValueError(f"image {image_id}: the stored arrays disagree on the number of ROIs")
        p["tm_shape"] = tm_shape
        cover = None

        def coverage(rows):
            nonlocal cover
            if cover is None:
                cover = self._coverage(p)
            return cover(rows)

        sel = select_head_rois(tci, coverage, self.T, self.config, self.rng, self.training)
        M, m = self.mask_pool, self.mask_size
        rois_aligned = headstore.unpack_gather(p["rois_aligned"], ra_shape, sel)
        mask_aligned = headstore.unpack_gather(p["mask_bits"], ma_shape, sel, (M, M, M))
        target_mask = headstore.unpack_gather(p["tm_bits"], tm_shape, sel, (m, m, m))[..., 0]
        idx = torch.from_numpy(sel).to(self.device)
        keep, idx = idx >= 0, idx.clamp(min=0)

        def take(a):                                    # _take_or_pad of a small array: padded rows zero
            a = torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
            if R == 0:
                return torch.zeros((self.T,) + tuple(a.shape[1:]), dtype=a.dtype, device=self.device)
            g = a.index_select(0, idx)
            return torch.where(keep.reshape((-1,) + (1,) * (g.dim() - 1)), g, torch.zeros_like(g))

        rois, ids, bbox = take(p["rois"]), take(tci), take(p["target_bbox"])
        H, W, D = self.shape
        meta = compose_image_meta(image_id, (H, W, D, 1), (H, W, D, 1), (0, 0, 0, H, W, D), 1.0,
                                  np.ones(self.num_classes, np.int32))
        self.last = {"image_id": image_id, "sel": sel, "rois": rois[None]}
        return [rois_aligned[None], mask_aligned[None], torch.from_numpy(meta[None]).to(self.device), ids[None],
                bbox[None], target_mask[None]]
