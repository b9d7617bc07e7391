"""The RPN training generator on the device.

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
