"""Fused Mask R-CNN head losses (m3d_head_loss_fwd / _bwd, m3d.head_losses)
against the float64 CPU evaluation of tests/headloss_ref.py (the torch
restatement of mrcnn_class_loss_graph / mrcnn_bbox_loss_graph /
mrcnn_mask_loss_graph, pinned by tests/test_headloss_ref.py): the three loss
values, the weighted total and the gradients w.r.t. the logits, the boxes and
the masks, every element compared.

Bars (the project's own, tests/test_gpu_rpn_loss.py): each loss within
2e-6 * max(1, |ref|), each gradient within 1e-6 of the reference gradient's
largest entry.  The restatement evaluated in float32 on the CPU stays within
1.7e-7 / 3.4e-7 of float64 at these shapes, so the bars leave about 10x / 3x
over plain float32 arithmetic.

Inputs: logits N(0,6), boxes N(0,2.5), box targets N(0,1.5), mask predictions
U(0,1), mask targets Bernoulli(0.3), the first half of each image's rows
background; on top, exact rows on the branch boundaries (see _case).  A random
row that lies close to a discontinuity is resampled (never dropped), so the
float32 kernel and the float64 checker take the same side of every branch.
"""
import functools

import numpy as np
import pytest
import torch

import headloss_ref as HL

pytestmark = pytest.mark.gpu

SHAPES = [
    (2, 64, 2, (6, 6, 5)),        # V = 180, not a multiple of 4 * 64
    (1, 37, 5, (7, 7, 7)),        # odd everything; general-C path; class 2 of image 0 inactive
    (2, 8, 2, (28, 28, 28)),      # the real V: several workgroups per row
    (1, 5, 4, (4, 4, 4)),         # the other vector path
]
WEIGHTS = (1.0, 1.5, 0.75)


def _near_class_discontinuity(logits, ids):
    """Rows whose float32 evaluation could take another branch than float64."""
    z = np.clip(logits.astype(np.float64), -10.0, 10.0)
    e = np.exp(z - z.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True)
    pt = np.take_along_axis(p, ids[:, None].astype(np.int64), 1)[:, 0]
    bad = np.abs(p[:, 1:].max(-1) - 0.5) < 1e-3
    bad |= np.abs(pt - 1e-7) < 1e-9
    bad |= (np.abs(np.abs(logits.astype(np.float64)) - 10.0) < 1e-4).any(-1)
    return bad


def _near_bbox_discontinuity(pred, target, ids):
    R = len(ids)
    y = 3.0 * np.tanh(pred.astype(np.float64)[np.arange(R), ids] / 3.0)
    return (np.abs(np.abs(target.astype(np.float64) - y) - 1.0) < 1e-4).any(-1) & (ids > 0)


@functools.lru_cache(maxsize=None)
def _case(B, T, C, ms, seed=0):
    """Host inputs (float32 numpy) of one shape.  Image 0's first rows are:
       bg 0   logits all 0: a tie, max foreground probability exactly 0.5 at C = 2
       bg 1   logits (0, 3, ...): a confident false positive
       pos 0  logits (10, -10, ...), target 1: p_t below eps; +-10 pass the gradient;
              its mask predictions start with exactly 0, 1 and 0.5
       pos 1  logits (12, -12, ...): clipped, gradient 0 there
       pos 2  an all-zero target mask (dropped from the mask loss)"""
    rng = np.random.default_rng(1000 * seed + 17 * T + C)
    R, V = B * T, int(np.prod(ms))
    half = T // 2
    assert half >= 2 and T - half >= 3
    ids = np.zeros((B, T), np.int32)
    ids[:, half:] = rng.integers(1, C, (B, T - half))
    ids[0, half] = 1
    active = np.ones((B, C), np.float32)
    if C == 5:
        active[0, 2] = 0.0
        ids[0, -1] = 2                                           # at least one row meets the inactive class
    logits = rng.normal(0, 6, (R, C)).astype(np.float32)
    bbox = rng.normal(0, 2.5, (R, C, 6)).astype(np.float32)
    tbox = rng.normal(0, 1.5, (R, 6)).astype(np.float32)
    mask = rng.uniform(0, 1, (R, V, C)).astype(np.float32)
    tmask = (rng.uniform(size=(R, V)) < 0.3).astype(np.float32)
    flat = ids.reshape(R)
    exact = np.zeros(R, bool)
    exact[[0, 1, half, half + 1]] = True
    logits[0] = 0.0
    logits[1, :2], logits[1, 2:] = [0.0, 3.0], -2.0
    logits[half, :2], logits[half, 2:] = [10.0, -10.0], 1.0
    logits[half + 1, :2], logits[half + 1, 2:] = [12.0, -12.0], -1.0
    mask[half, :3, :] = np.array([0.0, 1.0, 0.5], np.float32)[:, None]
    tmask[half, :3] = [1.0, 0.0, 1.0]
    tmask[half + 2] = 0.0
    for _ in range(100):                                         # resample, never drop
        bad = _near_class_discontinuity(logits, flat) & ~exact
        if not bad.any():
            break
        logits[bad] = rng.normal(0, 6, (int(bad.sum()), C)).astype(np.float32)
    else:
        raise AssertionError("class rows keep landing on a discontinuity")
    for _ in range(100):
        bad = _near_bbox_discontinuity(bbox, tbox, flat)
        if not bad.any():
            break
        bbox[bad] = rng.normal(0, 2.5, (int(bad.sum()), C, 6)).astype(np.float32)
    else:
        raise AssertionError("bbox rows keep landing on a discontinuity")
    keep = np.zeros_like(mask, bool)
    keep[half, :3, :] = True
    for _ in range(100):
        bad = ((mask < 1e-6) | (mask > 1.0 - 1e-6)) & ~keep
        if not bad.any():
            break
        mask[bad] = rng.uniform(0, 1, int(bad.sum())).astype(np.float32)
    else:
        raise AssertionError("mask predictions keep landing on a clip boundary")
    return dict(ids=ids, active=active, logits=logits.reshape(B, T, C), bbox=bbox.reshape(B, T, C, 6),
                tbox=tbox.reshape(B, T, 6), mask=mask.reshape((B, T) + ms + (C,)),
                tmask=tmask.reshape((B, T) + ms))


@functools.lru_cache(maxsize=None)
def _reference(B, T, C, ms):
    """Float64 CPU losses and gradients of the weighted total; computed once per shape."""
    c = _case(B, T, C, ms)
    x = [torch.tensor(c[k], dtype=torch.float64, requires_grad=True) for k in ("logits", "bbox", "mask")]
    out = HL.losses(torch.from_numpy(c["ids"]), torch.tensor(c["tbox"], dtype=torch.float64),
                    torch.tensor(c["tmask"], dtype=torch.float64), x[0], x[1], x[2],
                    torch.tensor(c["active"], dtype=torch.float64), WEIGHTS)
    out[0].backward()
    return [float(v.detach()) for v in out], [t.grad for t in x]


def _device_inputs(c, dev, grad=True):
    t = {k: torch.from_numpy(v).to(dev) for k, v in c.items()}
    for k in ("logits", "bbox", "mask"):
        t[k].requires_grad_(grad)
    return t


def _fused(t, weights=WEIGHTS, **kw):
    from m3d.head_losses import mrcnn_losses
    return mrcnn_losses(t["ids"], t["tbox"], t["tmask"], t["logits"], t["bbox"], t["mask"], t["active"], weights, **kw)


def _run(c, dev, weights=WEIGHTS, scale=1.0):
    t = _device_inputs(c, dev)
    out = _fused(t, weights)
    (out[0] * scale).backward() if scale != 1.0 else out[0].backward()
    return out, [t[k].grad for k in ("logits", "bbox", "mask")]


@pytest.mark.parametrize("B,T,C,ms", SHAPES)
def test_parity_with_the_float64_restatement(cuda, B, T, C, ms):
    ref_loss, ref_grad = _reference(B, T, C, ms)
    out, grads = _run(_case(B, T, C, ms), cuda)
    got = [float(v.detach()) for v in out]
    for name, a, b in zip(("total", "class", "bbox", "mask"), got, ref_loss):
        print(f"loss {name}: fused {a!r} ref {b!r} rel {abs(a - b) / max(1.0, abs(b)):.3g}")
    errs = []
    for name, ga, gb in zip(("logits", "bbox", "mask"), grads, ref_grad):
        gmax = float(gb.abs().max())
        err = float((ga.detach().double().cpu() - gb).abs().max())
        errs.append((name, err, gmax))
        print(f"grad {name}: max err {err:.3g} of max entry {gmax:.3g} -> {err / max(gmax, 1e-300):.3g}")
    assert ref_loss[1] > 0 and ref_loss[2] > 0 and ref_loss[3] > 0
    for a, b in zip(got, ref_loss):
        assert abs(a - b) <= 2e-6 * max(1.0, abs(b)), (a, b)
    for name, err, gmax in errs:
        assert gmax > 0 and err <= 1e-6 * gmax, (name, err, gmax)


def test_fractional_mask_targets(cuda):
    """Mask targets that are not 0 / 1: BCE and Dice with fractional y."""
    B, T, C, ms = SHAPES[3]
    c = dict(_case(B, T, C, ms))
    c["tmask"] = np.random.default_rng(3).uniform(0, 1, c["tmask"].shape).astype(np.float32)
    x = torch.tensor(c["mask"], dtype=torch.float64, requires_grad=True)
    ref = HL.mask_loss(torch.tensor(c["tmask"], dtype=torch.float64), torch.from_numpy(c["ids"]), x)
    ref.backward()
    t = _device_inputs(c, cuda)
    from m3d.head_losses import mrcnn_mask_loss
    got = mrcnn_mask_loss(t["tmask"], t["ids"], t["mask"])
    got.backward()
    assert abs(float(got.detach()) - float(ref.detach())) <= 2e-6 * max(1.0, abs(float(ref.detach())))
    err = float((t["mask"].grad.double().cpu() - x.grad).abs().max())
    assert err <= 1e-6 * float(x.grad.abs().max()), err


def test_all_background_targets(cuda):
    """The _no_pos branches: bbox and mask loss 0 with zero gradients, class loss finite."""
    c = dict(_case(*SHAPES[0]))
    c["ids"] = np.zeros_like(c["ids"])
    out, (gl, gb, gm) = _run(c, cuda)
    assert float(out[2]) == 0.0 and float(out[3]) == 0.0
    assert np.isfinite(float(out[1])) and float(out[1]) > 0
    assert float(gb.abs().max()) == 0.0 and float(gm.abs().max()) == 0.0
    assert torch.isfinite(gl).all() and float(gl.abs().max()) > 0
    ref = float(HL.class_loss(torch.from_numpy(c["ids"]), torch.tensor(c["logits"], dtype=torch.float64),
                              torch.tensor(c["active"], dtype=torch.float64)))
    assert abs(float(out[1]) - ref) <= 2e-6 * max(1.0, abs(ref))


def test_positives_with_empty_target_masks(cuda):
    """The _no_valid branch: every positive's target mask is empty -> mask loss 0, gradient 0."""
    c = dict(_case(*SHAPES[0]))
    c["tmask"] = np.zeros_like(c["tmask"])
    out, (_, gb, gm) = _run(c, cuda)
    assert float(out[3]) == 0.0 and float(gm.abs().max()) == 0.0
    assert float(out[2]) > 0 and float(gb.abs().max()) > 0


@pytest.mark.parametrize("B,T,C,ms", [SHAPES[0], SHAPES[1], SHAPES[3]])
def test_mask_gradient_is_written_whole(cuda, B, T, C, ms):
    """m3d_head_loss_bwd into a NaN-filled buffer: all finite, zero off the target channel."""
    from m3d import _lib
    L = _lib.load()
    c = _case(B, T, C, ms)
    t = _device_inputs(c, cuda, grad=False)
    R, V = B * T, int(np.prod(ms))
    sc = torch.empty(4, device=cuda)
    state = torch.empty(4 + 4 * R, device=cuda)
    ws = torch.empty(int(L.m3d_head_loss_workspace_bytes(R, V)), device=cuda, dtype=torch.uint8)
    p = _lib.ptr
    _lib.check(L.m3d_head_loss_fwd(None, None, p(t["mask"]), p(t["ids"]), None, p(t["tmask"]), None, B, T, C, V,
                                   0.85, 3.0, 1.0, 1.0, 1.0, sc[0].data_ptr(), sc[1].data_ptr(), sc[2].data_ptr(),
                                   sc[3].data_ptr(), p(state), p(ws), ws.numel(), _lib.stream()))
    g = torch.full((R, V, C), float("nan"), device=cuda)
    one = torch.ones((), device=cuda)
    _lib.check(L.m3d_head_loss_bwd(None, None, p(t["mask"]), p(t["ids"]), None, p(t["tmask"]), None, B, T, C, V,
                                   0.85, 3.0, p(state), p(one), None, None, p(g), _lib.stream()))
    assert torch.isfinite(g).all()
    ids = t["ids"].reshape(R).long()
    off = torch.ones((R, 1, C), device=cuda)
    off[torch.arange(R, device=cuda), 0, ids] = 0.0
    assert float((g * off).abs().max()) == 0.0
    assert float(g[ids == 0].abs().max()) == 0.0 and float(g.abs().max()) > 0
    # mask alone: class and bbox are skipped, total = the mask loss
    assert float(sc[1]) == 0.0 and float(sc[2]) == 0.0 and float(sc[0]) == float(sc[3]) > 0


def test_total_is_the_weighted_sum_and_upstream_scaling(cuda):
    c = _case(*SHAPES[0])
    out, grads = _run(c, cuda)
    tot, lc, lb, lm = (float(v.detach()) for v in out)
    want = lc * WEIGHTS[0] + lb * WEIGHTS[1] + lm * WEIGHTS[2]
    assert abs(tot - want) <= 1e-6 * max(1.0, abs(want))
    out3, grads3 = _run(c, cuda, scale=3.0)                      # (3 * total).backward()
    for g1, g3 in zip(grads, grads3):
        assert float((g3 - 3.0 * g1).abs().max()) <= 1e-6 * float(g3.abs().max())
    unit, _ = _run(c, cuda, weights=None)                        # the config's LOSS_WEIGHTS: 1.0 each
    assert abs(float(unit[0].detach()) - (lc + lb + lm)) <= 1e-6 * max(1.0, lc + lb + lm)


@pytest.mark.parametrize("B,T,C,ms", [SHAPES[0], SHAPES[2]])
def test_run_to_run_bit_identical(cuda, B, T, C, ms):
    c = _case(B, T, C, ms)
    out1, g1 = _run(c, cuda)
    out2, g2 = _run(c, cuda)
    assert all(torch.equal(a, b) for a, b in zip(out1, out2))
    assert all(torch.equal(a, b) for a, b in zip(g1, g2))


def test_single_loss_wrappers_equal_the_fused_call(cuda):
    from m3d.head_losses import mrcnn_bbox_loss, mrcnn_class_loss, mrcnn_mask_loss
    c = _case(*SHAPES[1])
    out, grads = _run(c, cuda, weights=(1.0, 1.0, 1.0))
    t = _device_inputs(c, cuda)
    lc = mrcnn_class_loss(t["ids"], t["logits"], t["active"])
    lb = mrcnn_bbox_loss(t["tbox"], t["ids"], t["bbox"])
    lm = mrcnn_mask_loss(t["tmask"][..., None], t["ids"], t["mask"])      # the reference's trailing 1 axis
    assert torch.equal(lc, out[1]) and torch.equal(lb, out[2]) and torch.equal(lm, out[3])
    (lc + lb + lm).backward()
    for k, g in zip(("logits", "bbox", "mask"), grads):
        assert torch.equal(t[k].grad, g)


def test_no_grad_and_cpu_tensors(cuda):
    from m3d.head_losses import active_class_ids_from_meta, mrcnn_losses
    c = _case(*SHAPES[3])
    t = _device_inputs(c, cuda)
    with torch.no_grad():
        out = _fused(t)
    assert not out[0].requires_grad and out[0].grad_fn is None
    ref, _ = _reference(*SHAPES[3])
    assert abs(float(out[0]) - ref[0]) <= 2e-6 * max(1.0, abs(ref[0]))
    h = {k: torch.from_numpy(v) for k, v in c.items()}
    with pytest.raises(ValueError, match="GPU"):
        mrcnn_losses(h["ids"], h["tbox"], h["tmask"], h["logits"], h["bbox"], h["mask"], h["active"])
    meta = torch.arange(2 * 18, dtype=torch.float32).reshape(2, 18)
    assert torch.equal(active_class_ids_from_meta(meta), meta[:, 16:])


def test_graph_capture_single_stream(cuda):
    """Forward + backward captured in one HIP graph on one stream, replayed once: bit-equal to eager."""
    c = _case(*SHAPES[0])
    eager_out, eager_g = _run(c, cuda)
    t = _device_inputs(c, cuda)
    keys = ("logits", "bbox", "mask")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                # warm up off the capture
        for _ in range(2):
            for k in keys:
                t[k].grad = None
            _fused(t)[0].backward()
    torch.cuda.current_stream().wait_stream(side)
    for k in keys:
        t[k].grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _fused(t)
        out[0].backward()
    for k in keys:
        t[k].grad.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, eager_out))
    assert all(torch.equal(t[k].grad, g) for k, g in zip(keys, eager_g))


def test_maskrcnn_head_losses_end_to_end(cuda):
    """MaskRCNN.head_losses at 64 x 64 x 8.  Ground truth: three cuboids of
    24-32 px across the full depth, class 1.  Thresholds: RPN_POSITIVE_IOU 0.1,
    RPN_NEGATIVE_IOU 0.05 -- with 300 proposals of an untrained RPN over a
    64 x 64 x 8 volume some overlap a cuboid of that size by IoU >= 0.1, so
    DetectionTargetLayer samples positives and the mask loss is non-zero."""
    from m3d.config import synthetic_mrcnn_config
    from m3d.head_losses import mrcnn_losses
    from m3d.heads import MaskRCNN
    from m3d.model import compose_image_meta, synthetic_volume
    cfg = synthetic_mrcnn_config(64, depth=8, PRE_NMS_LIMIT=2000, POST_NMS_ROIS_TRAINING=300,
                                 POST_NMS_ROIS_INFERENCE=64, TRAIN_ROIS_PER_IMAGE=12, ROI_POSITIVE_RATIO=0.5,
                                 RPN_POSITIVE_IOU=0.1, RPN_NEGATIVE_IOU=0.05, USE_MINI_MASK=False,
                                 MASK_SHAPE=[28, 28, 28], DETECTION_MAX_INSTANCES=8)
    model = MaskRCNN(cfg, device=cuda, seed=2)
    meta = torch.from_numpy(compose_image_meta(0, [64, 64, 8, 1], [64, 64, 8, 1], [0, 0, 0, 64, 64, 8], 1.0,
                                               [1, 1])[None]).to(cuda)
    boxes = np.array([[4, 4, 0, 32, 36, 8], [30, 8, 0, 60, 34, 8], [12, 36, 0, 40, 62, 8]], np.float32)
    masks = np.zeros((64, 64, 8, 3), bool)
    for g, (y1, x1, z1, y2, x2, z2) in enumerate(boxes.astype(int)):
        masks[y1:y2, x1:x2, z1:z2, g] = True
    gt_ids = torch.ones((1, 3), dtype=torch.int32, device=cuda)
    out = model.head_losses(synthetic_volume(64, 8).to(cuda), meta, gt_ids, torch.from_numpy(boxes[None]).to(cuda),
                            torch.from_numpy(masks[None]).to(cuda), seed=5)
    torch.cuda.synchronize()
    names = ("loss", "mrcnn_class_loss", "mrcnn_bbox_loss", "mrcnn_mask_loss")
    vals = [float(out[n]) for n in names]
    print(dict(zip(names, vals)), "positives", int((out["target_class_ids"] > 0).sum()))
    assert all(np.isfinite(v) for v in vals)
    assert out["mrcnn_mask"].shape == (1, 12, 28, 28, 28, 2) and out["target_mask"].shape == (1, 12, 28, 28, 28)
    assert vals[3] > 0.0, "no positive ROI was sampled"
    by_hand = mrcnn_losses(out["target_class_ids"], out["target_bbox"], out["target_mask"],
                           out["mrcnn_class_logits"], out["mrcnn_bbox"], out["mrcnn_mask"],
                           out["active_class_ids"], out["loss_weights"])
    assert all(torch.equal(out[n], v) for n, v in zip(names, by_hand))
