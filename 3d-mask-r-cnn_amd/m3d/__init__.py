"""m3d -- MI355X-native (gfx950) hot path of podtyazhki1337/3d-mask-r-cnn.

Drop-in surface:
  m3d.ops      crop_and_resize_3d / _grad_image / _grad_boxes, non_max_suppression_3d,
               pyramid_roi_align (core/custom_op/custom_op.py:22-65)
  m3d.layers   ProposalLayer, PyramidROIAlign (core/models.py:369-503, 597-687)
  m3d.backbone ResNet3D (resnet_graph), FPN, RPNHead (build_rpn_model)
  m3d.model    RPN training model, losses, synthetic inputs
  m3d.heads    classifier / mask heads, DetectionLayer, MaskRCNN (detect, head_losses)
  m3d.head_losses  mrcnn_losses (+ mrcnn_class_loss / mrcnn_bbox_loss / mrcnn_mask_loss,
               active_class_ids_from_meta): core/models.py:1676-1960, value + gradient
  m3d.headstore  the stored head targets of TARGET_GENERATION (core/models.py:3530-3796): float16 /
               bit-packed forms made and read back on the GPU; ToyHeadDataset (m3d.dataset),
               HeadGenerator (m3d.generator), MaskRCNN.head_target_generation / train_heads_on_features
  m3d.rpn_eval   RPN_EVALUATION (core/utils.py:1251-1415): score_proposals (proposals against GT boxes on the
               GPU), summarize (the callback's numbers on the host); RPN.evaluate (m3d.model) is the loop
  m3d.config   Config / load_config (core/config.py)
  m3d.parallel depth-slab sharding + RCCL gradient all-reduce
All compute runs in libm3d.so (hand-written HIP for gfx950); there is no CPU
fallback.
"""
from . import config  # noqa: F401

__all__ = ["config", "ops", "layers", "backbone", "model", "anchors", "heads", "head_losses", "mrcnn_losses",
           "mrcnn_class_loss", "mrcnn_bbox_loss", "mrcnn_mask_loss", "active_class_ids_from_meta"]

_HEAD_LOSS_NAMES = ("mrcnn_losses", "mrcnn_class_loss", "mrcnn_bbox_loss", "mrcnn_mask_loss",
                    "active_class_ids_from_meta")


def __getattr__(name):
    """The head-loss names resolve on first use (importing m3d itself stays free of torch)."""
    if name in _HEAD_LOSS_NAMES:
        from . import head_losses
        return getattr(head_losses, name)
    raise AttributeError(f"module 'm3d' has no attribute {name!r}")
