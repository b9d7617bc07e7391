"""The segmentation volume, its pixelwise counts and the TIFF page order on the
GPU (m3d_unmold_labels, m3d_label_pixelwise, m3d_labels_stack; m3d.evaluate,
MaskRCNN.evaluate / evaluate_dataset) against the numpy restatement
tests/segref.py (pinned by tests/test_segref.py).

Bars: every output is an integer and equals the restatement bit for bit; the
host metrics are the restatement's float64 arithmetic and equal it exactly.

Shapes: the twelve detections of tests/unmoldref.py (one row per status code)
at 24 x 20 x 16 and at the all-odd 23 x 19 x 15, m = 28 and m = 8 -- their
masks overlap, so a voxel's label depends on which detection wins; one case at
128 x 128 x 64 with three boxes of about 100 x 100 x 50 (64 workgroups per
detection meet on shared voxels); G = 0, 1, 3, 17 and 1030 for the counts (no
GT, a tail group alone, 4-byte groups plus a tail, more groups than a
workgroup has lanes) and G = 6, 50 and 1024 (a tail dword that overlaps the
group before it by two bytes, the timing script's shape, every lane of the
workgroup on one voxel), one case with G = 4200 at 128 x 128 x 64 whose byte
offsets pass 2^32; (7, 5, 1) for a stack with a single page."""
import bz2
import csv
import functools
import os
import pickle

import numpy as np
import pytest
import torch

import segref as S
import unmoldref as U

pytestmark = pytest.mark.gpu

SHAPE = U.SHAPE
ODD = (23, 19, 15)
BIG = (128, 128, 64)


def _np(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _ref(m, C, shape=SHAPE):
    det, mask = U.case(m, C)
    return det, mask, U.unmold(det, mask, shape)


@functools.lru_cache(maxsize=None)
def _big():
    """Three boxes of 104 x 101 x 52, 98 x 98 x 49 and 98 x 98 x 49 voxels in
    128 x 128 x 64, overlapping pairwise: a nearly full one, then two balls
    painted over it and over each other."""
    grids = U.case_grids(28, seed=3)
    det = np.zeros((4, 8), np.float32)
    det[0] = [0.1, 0.12, 0.1, 0.9, 0.9, 0.9, 1, 0.9]
    det[1] = [0.0, 0.0, 0.0, 0.76, 0.76, 0.76, 1, 0.8]
    det[3] = [0.24, 0.24, 0.24, 1.0, 1.0, 1.0, 1, 0.7]          # (row 2 is padding)
    mask = np.zeros((4, 28, 28, 28, 2), np.float32)
    mask[0, ..., 1], mask[1, ..., 1], mask[3, ..., 1] = grids["dense_high"], grids["clean_otsu"], grids["clean_otsu"]
    r = U.unmold(det, mask, BIG)
    assert r["status"].tolist() == [U.OK, U.OK, U.NOT_KEPT, U.OK]
    ext = r["box_i"][:, 3:] - r["box_i"][:, :3]
    assert (ext[[0, 1, 3]] >= (96, 96, 48)).all()
    d = r["dense"].astype(bool)
    assert all((d[a] & d[b]).sum() > 1000 for a, b in ((0, 1), (0, 3), (1, 3)))
    seg, label_of = S.labels(r["dense"], r["status"])
    return det, mask, r, seg, label_of


def _unmold(cuda, det, mask, shape, **kw):
    from m3d import evaluate as E
    return E.unmold_detections(torch.from_numpy(det).to(cuda), torch.from_numpy(mask).to(cuda), shape, **kw)


def _coverage(r):
    """How many masks cover each voxel (rejected rows are all zero)."""
    return r["dense"].astype(np.int32).sum(0)


@pytest.mark.parametrize("m,C,shape", [(28, 2, SHAPE), (8, 1, SHAPE), (28, 2, ODD), (8, 1, ODD)])
def test_labels_equal_the_restatement(cuda, m, C, shape):
    det, mask, r = _ref(m, C, shape)
    seg, label_of = S.labels(r["dense"], r["status"])
    cov = _coverage(r)
    print("voxels covered >= 2x:", int((cov >= 2).sum()), ">= 3x:", int((cov >= 3).sum()))
    if shape == SHAPE:                                          # the precondition, on the restatement itself
        assert (cov >= 2).sum() >= 100 and (cov >= 3).sum() >= 10
        if m == 28:                                             # one lower label is fully hidden
            hidden = [k for k in label_of[r["area_pred"] > 0] if k not in seg]
            assert hidden and max(hidden) < label_of.max()
    u = _unmold(cuda, det, mask, shape, union=True, labels=True)
    assert u.labels.dtype == torch.int32 and tuple(u.labels.shape) == shape and u.label_of.dtype == torch.int32
    assert np.array_equal(_np(u.label_of), label_of)
    assert np.array_equal(_np(u.labels), seg)
    assert np.array_equal(_np(u.labels) > 0, _np(u.seg_union) > 0) and np.array_equal(_np(u.seg_union), r["seg_union"])
    # the listed rows in label order are compact()'s rows (the RANGE row dropped so that it does not raise)
    keep = np.array([n != "range" for n in U.ROWS])
    u2 = _unmold(cuda, det[keep], mask[keep], shape, labels=True)
    rows = u2.compact()["rows"]
    assert np.array_equal(_np(u2.label_of)[rows], np.arange(1, len(rows) + 1))
    assert np.count_nonzero(_np(u2.label_of)) == len(rows)
    # without the flag nothing is built
    u3 = _unmold(cuda, det, mask, shape)
    assert u3.labels is None and u3.label_of is None


@pytest.mark.parametrize("m,C,shape", [(28, 2, SHAPE), (8, 1, ODD)])
def test_keep_filters_the_list(cuda, m, C, shape):
    """keep drops the last row (clean_otsu, the top label) and one middle row:
    the rows after a dropped one move up, what the top label hid shows through."""
    det, mask, r = _ref(m, C, shape)
    keep = np.ones(len(U.ROWS), bool)
    keep[[U.ROWS.index("clean_otsu"), U.ROWS.index("thin_percentile")]] = False
    seg, label_of = S.labels(r["dense"], r["status"], keep)
    full, _ = S.labels(r["dense"], r["status"])
    assert (seg > 0).sum() < (full > 0).sum() and label_of.max() == full.max() - 2
    for k in (torch.from_numpy(keep), torch.from_numpy(keep.astype(np.uint8))):
        u = _unmold(cuda, det, mask, shape, labels=True, keep=k.to(cuda))
        assert np.array_equal(_np(u.label_of), label_of) and np.array_equal(_np(u.labels), seg)
    none = _unmold(cuda, det, mask, shape, labels=True, keep=torch.zeros(len(U.ROWS), dtype=torch.bool, device=cuda))
    assert not none.labels.any() and not none.label_of.any()
    with pytest.raises(ValueError, match="keep"):
        _unmold(cuda, det, mask, shape, labels=True, keep=torch.ones(5, dtype=torch.bool, device=cuda))
    with pytest.raises(ValueError, match="labels=True"):
        _unmold(cuda, det, mask, shape, keep=torch.from_numpy(keep).to(cuda))


def test_many_workgroups_meet_on_shared_voxels(cuda):
    det, mask, r, seg, label_of = _big()
    u = _unmold(cuda, det, mask, BIG, labels=True)
    assert np.array_equal(_np(u.label_of), label_of) and label_of.tolist() == [1, 2, 0, 3]
    assert np.array_equal(_np(u.labels), seg)
    assert all((seg == k).sum() > 1000 for k in (1, 2, 3))       # (checked on the restatement: 344052, 96836, 111166)


def test_guard_bands_stay_intact(cuda):
    """labels, label_of, stack and counts as interior slices of sentinel-filled
    buffers at the all-odd volume: every byte around them survives."""
    import m3d._lib as lib
    L, p, s = lib.load(), lib.ptr, lib.stream()
    det, mask, r = _ref(8, 1, ODD)
    seg, label_of = S.labels(r["dense"], r["status"])
    gt = U.case_gt(3, ODD)
    u = _unmold(cuda, det, mask, ODD)
    H, W, D = ODD
    V, n, pad = H * W * D, len(U.ROWS), 7
    i32 = lambda size: torch.full((size + 2 * pad,), 0x5A5A5A5A, dtype=torch.int32, device=cuda)    # noqa: E731
    lab_buf, lof_buf = i32(V), i32(n)
    cnt_buf = torch.full((5,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=cuda)
    st8 = torch.full((V + 2 * pad,), 0x5A, dtype=torch.uint8, device=cuda)
    st16 = torch.full((V + 2 * pad,), 0x5A5A, dtype=torch.int16, device=cuda)
    labels, lof, counts = lab_buf[pad:pad + V].view(H, W, D), lof_buf[pad:pad + n], cnt_buf[1:4]
    lib.check(L.m3d_unmold_labels(p(u.small), p(u.box_i), p(u.status), p(u.stats), None, n, u.m, H, W, D, p(lof),
                                  p(labels), s))
    g = torch.from_numpy(gt).to(cuda)
    lib.check(L.m3d_label_pixelwise(p(labels), p(g), H, W, D, 3, p(counts), s))
    lib.check(L.m3d_labels_stack(p(labels), H, W, D, 1, p(st8[pad:pad + V]), s))
    lib.check(L.m3d_labels_stack(p(labels), H, W, D, 2, p(st16[pad:pad + V]), s))
    torch.cuda.synchronize()
    assert np.array_equal(_np(labels), seg) and np.array_equal(_np(lof), label_of)
    assert tuple(_np(counts).tolist()) == S.pixelwise_counts(seg, gt)
    want = np.moveaxis(seg, -1, 0)
    assert np.array_equal(_np(st8[pad:pad + V]).reshape(D, H, W), want.astype(np.uint8))
    assert np.array_equal(_np(st16[pad:pad + V]).reshape(D, H, W), want.astype(np.int16))
    for buf, size in ((lab_buf, V), (lof_buf, n), (st8, V), (st16, V)):
        b = _np(buf.view(torch.uint8))
        w = buf.element_size()
        assert (b[:pad * w] == 0x5A).all() and (b[(pad + size) * w:] == 0x5A).all()
    b = _np(cnt_buf.view(torch.uint8))
    assert (b[:8] == 0x5A).all() and (b[32:] == 0x5A).all()


def _gt(G, shape=SHAPE):
    return U.case_gt(G, shape) if G else np.zeros(shape + (0,), np.uint8)


@pytest.mark.parametrize("G", [0, 1, 3, 6, 17, 50, 1024, 1030])
def test_pixelwise_counts_equal_numpy(cuda, G):
    from m3d import evaluate as E
    det, mask, r = _ref(8, 2)
    seg, _ = S.labels(r["dense"], r["status"])
    labels = torch.from_numpy(seg).to(cuda)
    gts = [_gt(G)]
    if G > 3:                                                   # single columns: the first byte, the last full group, the tail
        for col, region in ((0, np.s_[2:9]), (4 * ((G - 1) // 4) - 1, np.s_[8:15]), (G - 1, np.s_[13:22])):
            g = np.zeros(SHAPE + (G,), np.uint8)
            g[region, 3:17, 1:15, col] = 200
            gts.append(g)
    for i, gt in enumerate(gts):
        want = S.pixelwise_counts(seg, gt)
        got = E.pixelwise_counts(labels, torch.from_numpy(gt).to(cuda))
        assert got.dtype == torch.int64 and tuple(got.shape) == (3,)
        assert tuple(_np(got).tolist()) == want, (G, _np(got), want)
        assert sum(want) > 0 and (i == 0 or min(want) > 0)       # a single column leaves all three counts non-zero
    if G:                                                       # bool GT masks are read in place
        got = E.pixelwise_counts(labels, torch.from_numpy(gts[0].astype(bool)).to(cuda))
        assert tuple(_np(got).tolist()) == S.pixelwise_counts(seg, gts[0])
    empty = E.pixelwise_counts(torch.zeros_like(labels), torch.from_numpy(gts[0]).to(cuda))
    assert tuple(_np(empty).tolist()) == S.pixelwise_counts(np.zeros_like(seg), gts[0])


def test_pixelwise_gt_offsets_past_32_bits(cuda):
    """128 x 128 x 64 with G = 4200: a voxel's GT row starts at byte lin * G,
    past 2^32 from y = 125 on.  Seven columns are set -- the first and last of
    1024-byte stretches and the row's last byte -- each over its own y range, the
    rest are zero; built on the device.  A truncated offset reads other voxels."""
    from m3d import evaluate as E
    seg = _big()[3].copy()
    seg[120:128, 30:100, 10:50] = 7                             # labelled voxels where the offsets pass 2^32
    G = 4200
    cols = [0, 1023, 1024, 4095, 4096, 4199, 2048]
    spans = [(3, 17), (20, 33), (36, 50), (52, 66), (70, 85), (88, 101), (124, 128)]
    assert (125 * 128 * 64) * G > 2 ** 32
    small = np.zeros(BIG + (len(cols),), np.uint8)
    gt = torch.zeros(BIG + (G,), dtype=torch.uint8, device=cuda)
    for k, (col, (y0, y1)) in enumerate(zip(cols, spans)):
        small[y0:y1, 10:120, 5:60, k] = 1
        gt[y0:y1, 10:120, 5:60, col] = 1
    want = S.pixelwise_counts(seg, small)
    assert min(want) > 1000 and (seg[124:128, 10:120, 5:60] > 0).any() and (seg[124:128, 10:120, 5:60] == 0).any()
    got = E.pixelwise_counts(torch.from_numpy(seg).to(cuda), gt)
    assert tuple(_np(got).tolist()) == want


@pytest.mark.parametrize("shape", [SHAPE, ODD, (7, 5, 1), BIG])
def test_label_stack_is_the_page_order(cuda, shape):
    """Both sample widths through the C-ABI on arbitrary int32 labels (some
    past 16 bits: the narrowing truncates, as numpy's astype)."""
    import m3d._lib as lib
    L, p, s = lib.load(), lib.ptr, lib.stream()
    H, W, D = shape
    rng = np.random.default_rng(H * W + D)
    labels = rng.integers(0, 70000, shape).astype(np.int32)
    labels[rng.uniform(size=shape) < 0.5] = 0
    dev = torch.from_numpy(labels).to(cuda)
    for bps, tdt, ndt in ((1, torch.uint8, np.uint8), (2, torch.uint16, np.uint16)):
        out = torch.empty((D, H, W), dtype=tdt, device=cuda)
        out.view(torch.uint8).fill_(0x77)
        lib.check(L.m3d_labels_stack(p(dev), H, W, D, bps, p(out), s))
        assert np.array_equal(_np(out), np.moveaxis(labels, -1, 0).astype(ndt)), (shape, bps)


def test_label_stack_width_follows_max_inst(cuda):
    """12 rows -> uint8; 300 rows (the ten listed rows of the case tiled 30
    times: labels up to 300, which one byte would truncate) -> uint16."""
    det, mask, r = _ref(8, 1)
    u = _unmold(cuda, det, mask, SHAPE, labels=True)
    st = u.label_stack()
    assert st.dtype == torch.uint8 and tuple(st.shape) == (SHAPE[2], SHAPE[0], SHAPE[1])
    assert np.array_equal(_np(st), np.moveaxis(_np(u.labels), -1, 0).astype(np.uint8))
    sel = r["status"] != U.NOT_KEPT
    det, mask = np.tile(det[sel], (30, 1)), np.tile(mask[sel], (30, 1, 1, 1, 1))
    seg, label_of = S.labels(np.tile(r["dense"][sel], (30, 1, 1, 1)), np.tile(r["status"][sel], 30))
    assert len(det) == 300 and label_of.max() == 300 and seg.max() == 300
    u = _unmold(cuda, det, mask, SHAPE, labels=True)
    assert np.array_equal(_np(u.label_of), label_of) and np.array_equal(_np(u.labels), seg)
    st = u.label_stack()
    assert st.dtype == torch.uint16 and np.array_equal(_np(st), np.moveaxis(seg, -1, 0).astype(np.uint16))
    with pytest.raises(ValueError, match="labels=True"):
        _unmold(cuda, det, mask, SHAPE).label_stack()


def _chain(cuda, d, k, gt):
    """prepare -> overlaps -> areas -> finalize -> labels -> pixelwise -> stack."""
    from m3d import evaluate as E
    u = E.unmold_detections(d, k, SHAPE, gt_masks=gt, labels=True)
    return u, E.pixelwise_counts(u.labels, gt), u.label_stack()


def test_two_runs_are_bit_identical(cuda):
    det, mask, r = _ref(28, 2)
    d, k = torch.from_numpy(det).to(cuda), torch.from_numpy(mask).to(cuda)
    gt = torch.from_numpy(U.case_gt(17)).to(cuda)
    (u1, c1, s1), (u2, c2, s2) = _chain(cuda, d, k, gt), _chain(cuda, d, k, gt)
    torch.cuda.synchronize()
    assert torch.equal(u1.labels, u2.labels) and torch.equal(u1.label_of, u2.label_of)
    assert torch.equal(c1, c2) and torch.equal(s1, s2) and u1.labels.any()


def test_graph_capture_and_replay(cuda):
    det, mask, r = _ref(28, 2)
    gt_h = U.case_gt(17)
    seg, label_of = S.labels(r["dense"], r["status"])
    d, k, gt = torch.from_numpy(det).to(cuda), torch.from_numpy(mask).to(cuda), torch.from_numpy(gt_h).to(cuda)
    eager = _chain(cuda, d, k, gt)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _chain(cuda, d, k, gt)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        u, counts, stack = _chain(cuda, d, k, gt)
    for t in (u.labels, u.label_of, counts, u.status, u.area_pred):
        t.fill_(-1)
    stack.fill_(0xFF)
    u.small.fill_(0xFF)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_np(u.labels), seg) and np.array_equal(_np(u.label_of), label_of)
    assert tuple(_np(counts).tolist()) == S.pixelwise_counts(seg, gt_h)
    assert np.array_equal(_np(stack), np.moveaxis(seg, -1, 0).astype(np.uint8))
    assert torch.equal(u.labels, eager[0].labels) and torch.equal(counts, eager[1]) and torch.equal(stack, eager[2])
    assert torch.equal(u.overlaps[1], eager[0].overlaps[1])


def test_evaluate_detections_with_labels(cuda):
    """evaluate_detections(labels=True[, keep]) on the committed case (without
    its RANGE row): the new keys equal the restatement, the old ones equal the
    default call; keep restricts every per-row result."""
    from m3d import evaluate as E
    det, mask, r = _ref(8, 2)
    sel = np.array([n != "range" for n in U.ROWS])
    det, mask = det[sel], mask[sel]
    status, dense, area = r["status"][sel], r["dense"][sel], r["area_pred"][sel]
    gt = np.concatenate([U.case_gt(3), np.zeros(SHAPE + (2,), np.uint8)], -1)
    gt[..., 3] = dense[-1]
    gt[..., 4] = dense[2]
    gt[:6, :, :, 4] = 0
    gt_ids = np.array([1, 1, 1, 2, 1], np.int32)
    d, k, g = torch.from_numpy(det).to(cuda), torch.from_numpy(mask).to(cuda), torch.from_numpy(gt).to(cuda)
    base = E.evaluate_detections(d, k, SHAPE, gt_ids, g)
    assert sorted(base) == sorted(["mAP", "precision", "recall", "ious", "iou", "inter", "boxes", "scores",
                                   "class_ids", "rows", "status", "area_pred", "area_gt", "unmolded"])
    assert base["unmolded"].labels is None
    for keep in (None, np.array([n not in ("clean_otsu", "thin_percentile") for n in np.array(U.ROWS)[sel]])):
        out = E.evaluate_detections(d, k, SHAPE, gt_ids, g, labels=True,
                                    keep=None if keep is None else torch.from_numpy(keep).to(cuda))
        rows = S.listed_rows(status, keep)
        seg, label_of = S.labels(dense, status, keep)
        masks = S.listed_masks(dense, status, keep)
        assert np.array_equal(out["rows"], rows) and np.array_equal(out["label_of"], label_of)
        assert np.array_equal(_np(out["labels"]), seg)
        counts = S.pixelwise_counts(seg, gt)
        assert out["pixelwise_counts"] == counts and out["pixelwise"] == S.pixelwise_metrics(*counts)
        assert out["instance_dice"] == S.instance_dice(masks, gt)
        assert out["detection_performance"] == S.detection_performance(masks, gt)
        assert np.array_equal(out["area_pred"], area[rows]) and len(out["boxes"]) == len(rows)
        inter, area_gt = U.overlaps(dense, gt)
        assert np.array_equal(out["inter"], inter[rows])
        want = U.compute_ap(U.iou_matrix(inter, area, area_gt)[rows], det[rows, 6].astype(np.int32), gt_ids)
        assert (out["mAP"], out["precision"], out["recall"]) == want[:3]
        if keep is None:
            assert out["instance_dice"][2] == 2 and out["detection_performance"]["tp"] == 2
            for key in base:
                if key != "unmolded":
                    assert np.array_equal(np.asarray(out[key]), np.asarray(base[key]), equal_nan=True), key
        else:
            assert out["instance_dice"][2] == 1 and out["detection_performance"]["fn"] == 4
    # no ground truth at all
    out = E.evaluate_detections(d, k, SHAPE, np.zeros(0, np.int32), torch.from_numpy(gt[..., :0].copy()).to(cuda),
                                labels=True)
    seg, _ = S.labels(dense, status)
    assert out["pixelwise_counts"] == (0, int((seg > 0).sum()), 0) and out["instance_dice"] == (0.0, 0.0, 0)
    assert out["detection_performance"]["fp"] == len(out["rows"]) and np.array_equal(_np(out["labels"]), seg)


S64 = 64


@pytest.fixture(scope="module")
def toy_model(cuda):
    """The toy 64^3 configuration of test_maskrcnn_evaluate_end_to_end (same seed and overrides)."""
    from m3d.config import synthetic_mrcnn_config
    from m3d.heads import MaskRCNN
    cfg = synthetic_mrcnn_config(S64, PRE_NMS_LIMIT=2000, POST_NMS_ROIS_INFERENCE=64, DETECTION_MAX_INSTANCES=8,
                                 DETECTION_MIN_CONFIDENCE=0.0, MASK_SHAPE=[28, 28, 28])
    return MaskRCNN(cfg, device=cuda, seed=2)


def _toy_gt():
    boxes = np.array([[4, 4, 8, 32, 36, 40], [30, 8, 20, 60, 34, 60], [12, 36, 0, 40, 62, 30]], np.float32)
    gt = np.zeros((S64, S64, S64, 3), np.uint8)
    for g, (y1, x1, z1, y2, x2, z2) in enumerate(boxes.astype(int)):
        gt[y1:y2, x1:x2, z1:z2, g] = 1
    return boxes, gt


def _check_against_restatement(out, gt):
    """The label keys of one evaluate(labels=True) result against the restatement fed with detect's own outputs."""
    det, mask = _np(out["detections"][0]), _np(out["mrcnn_mask"][0])
    r = U.unmold(det, mask, (S64,) * 3)
    seg, label_of = S.labels(r["dense"], r["status"])
    masks = S.listed_masks(r["dense"], r["status"])
    assert np.array_equal(_np(out["labels"]), seg) and np.array_equal(out["label_of"], label_of)
    counts = S.pixelwise_counts(seg, gt)
    assert out["pixelwise_counts"] == counts and out["pixelwise"] == S.pixelwise_metrics(*counts)
    assert out["instance_dice"] == S.instance_dice(masks, gt)
    assert out["detection_performance"] == S.detection_performance(masks, gt)
    return r, seg


def test_maskrcnn_evaluate_with_labels(cuda, toy_model):
    from m3d.model import compose_image_meta, synthetic_volume
    S_ = S64
    meta = torch.from_numpy(compose_image_meta(0, [S_, S_, S_, 1], [S_, S_, S_, 1], [0, 0, 0, S_, S_, S_], 1.0,
                                               [1, 1])[None]).to(cuda)
    image = synthetic_volume(S_).to(cuda)
    boxes, gt = _toy_gt()
    args = (image, meta, torch.ones(3, dtype=torch.int32, device=cuda), torch.from_numpy(boxes[None]).to(cuda),
            torch.from_numpy(gt).to(cuda))
    base = toy_model.evaluate(*args)
    out = toy_model.evaluate(*args, labels=True)
    r, seg = _check_against_restatement(out, gt)
    print("status", r["status"].tolist(), "pixelwise", out["pixelwise"], "dice", out["instance_dice"])
    assert (r["status"] == U.OK).any() and seg.any(), "no detection of the random-weight model kept a mask"
    # the default call: the same keys as before, and the same values in both calls
    assert sorted(base) == sorted(["mAP", "precision", "recall", "ious", "iou", "inter", "boxes", "scores",
                                   "class_ids", "rows", "status", "area_pred", "area_gt", "unmolded", "detections",
                                   "mrcnn_mask"])
    assert base["unmolded"].labels is None
    for key in base:
        if key == "unmolded":
            continue
        a, b = (_np(v) if torch.is_tensor(v) else np.asarray(v) for v in (base[key], out[key]))
        assert np.array_equal(a, b, equal_nan=True), key


def _write_volume(root, name, seed):
    """One 64^3 volume in the reference's on-disk layout: (Z,Y,X) TIFF, .dat rows
    `class z1 y1 x1 z2 y2 x2`, bz2-pickled (Z,Y,X,N) masks."""
    from m3d.tiff import imwrite
    rng = np.random.default_rng(seed)
    boxes, gt = _toy_gt()
    if seed % 2:
        boxes, gt = boxes[:2], gt[..., :2]
    image = rng.integers(0, 256, (S64,) * 3).astype(np.uint8)                   # (Y,X,Z)
    image[gt.any(-1)] //= 2
    paths = [os.path.join(root, name + ext) for ext in (".tiff", ".dat", ".pickle.bz2")]
    imwrite(paths[0], np.transpose(image, (2, 0, 1)))
    with open(paths[1], "w") as f:
        for y1, x1, z1, y2, x2, z2 in boxes.astype(int):
            f.write(f"1 {z1} {y1} {x1} {z2} {y2} {x2}\n")
    with bz2.BZ2File(paths[2], "wb") as f:
        pickle.dump(np.transpose(gt.astype(bool), (2, 0, 1, 3)), f)
    return paths, gt


def test_evaluate_dataset(cuda, toy_model, tmp_path):
    from m3d.dataset import ToyDataset
    from m3d.model import compose_image_meta
    from m3d.tiff import imread
    root = str(tmp_path)
    os.makedirs(os.path.join(root, "datasets"))
    vols = [_write_volume(root, name, seed) for name, seed in (("vol_a", 4), ("vol_b", 5))]
    with open(os.path.join(root, "datasets", "test.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["images", "cabs", "masks"])
        for paths, _ in vols:
            w.writerow(paths)
    ds = ToyDataset()
    ds.load_dataset(root, is_train=False)
    ds.prepare()
    res_dir = os.path.join(root, "results")
    rep = toy_model.evaluate_dataset(ds, result_dir=res_dir)
    assert [r["name"] for r in rep["rows"]] == ["vol_a", "vol_b"]
    meta = torch.from_numpy(compose_image_meta(0, [S64] * 3 + [1], [S64] * 3 + [1], [0, 0, 0] + [S64] * 3, 1.0,
                                               [1, 1])[None]).to(cuda)
    for i, ((paths, gt), row) in enumerate(zip(vols, rep["rows"])):
        image = torch.from_numpy(ds.load_image(i)[None]).to(cuda)
        meta[0, 0] = i
        out = toy_model.evaluate(image, meta, np.ones(gt.shape[-1], np.int32), None, torch.from_numpy(gt).to(cuda),
                                 labels=True)
        _, seg = _check_against_restatement(out, gt)
        px, dice, det = out["pixelwise"], out["instance_dice"], out["detection_performance"]
        ious = np.asarray(out["ious"], np.float32)
        want = {"name": ("vol_a", "vol_b")[i], "pred_inst": len(out["rows"]), "ap50": out["mAP"],
                "prec50": out["precision"], "rec50": out["recall"],
                "miou": float(np.nanmean(ious)) if ious.size else 0.0, "px_precision": px[0], "px_recall": px[1],
                "px_f1": px[2], "px_iou": px[3], "dice_mean": dice[0], "dice_std": dice[1], "dice_n": dice[2],
                "det_tp": det["tp"], "det_fp": det["fp"], "det_fn": det["fn"], "det_recall": det["recall"],
                "det_precision": det["precision"]}
        assert list(row) == list(want)
        for key in want:
            assert row[key] == want[key] or (row[key] != row[key] and want[key] != want[key]), (key, row, want)
        stack = imread(os.path.join(res_dir, row["name"] + ".tiff"))
        assert stack.dtype == np.uint8 and np.array_equal(stack, np.moveaxis(seg, -1, 0).astype(np.uint8))
        lines = list(csv.reader(open(os.path.join(res_dir, row["name"] + ".csv"), newline="")))
        assert lines[0] == ["class", "y1", "x1", "z1", "y2", "x2", "z2"] and len(lines) == 1 + len(out["rows"])
        assert [int(r[0]) for r in lines[1:]] == out["class_ids"].tolist()
        assert np.array_equal(np.array([r[1:] for r in lines[1:]], np.float32).reshape(-1, 6), out["boxes"])
    rows = rep["rows"]
    assert rep["summary"] == {
        "images": 2, "pixelwise_f1_mean": float(np.mean([r["px_f1"] for r in rows])),
        "pixelwise_f1_std": float(np.std([r["px_f1"] for r in rows])),
        "instance_dice_mean": float(np.mean([r["dice_mean"] for r in rows])),
        "instance_dice_std": float(np.std([r["dice_mean"] for r in rows])),
        "recall_mean": float(np.mean([r["det_recall"] for r in rows])),
        "precision_mean": float(np.mean([r["det_precision"] for r in rows]))}
    # image_ids picks images; without result_dir nothing is written
    one = toy_model.evaluate_dataset(ds, image_ids=[1])
    assert [r["name"] for r in one["rows"]] == ["vol_b"] and one["rows"][0] == rows[1]
    assert sorted(os.listdir(res_dir)) == ["vol_a.csv", "vol_a.tiff", "vol_b.csv", "vol_b.tiff"]
    # a volume of another shape is refused, not resized
    from m3d.tiff import imwrite
    imwrite(vols[0][0][0], np.zeros((32, S64, S64), np.uint8))
    with pytest.raises(ValueError, match="does not resize"):
        toy_model.evaluate_dataset(ds, image_ids=[0])
