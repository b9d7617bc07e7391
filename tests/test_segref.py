"""tests/segref.py pinned with hand-derived answers, m3d.evaluate's host metric
functions held against it bit for bit, the TIFF writer against m3d.tiff.imread
and PIL, and the CSV format.  No GPU."""
import csv
import functools

import numpy as np
import pytest

import segref as S
import unmoldref as U


def _cuboids():
    """Five rows in a 4 x 4 x 4 volume: a padding row, cuboid A = [0:3]^3, a
    rejected (all-zero) row, cuboid B = [1:4]^3 and the slab C = [:, :, 2]."""
    dense = np.zeros((5, 4, 4, 4), np.uint8)
    dense[1, 0:3, 0:3, 0:3] = 1
    dense[3, 1:4, 1:4, 1:4] = 1
    dense[4, :, :, 2] = 1
    status = np.array([U.NOT_KEPT, U.OK, U.FLAT, U.OK, U.OK], np.int32)
    return dense, status


def test_label_map_of_three_overlapping_cuboids():
    dense, status = _cuboids()
    seg, label_of = S.labels(dense, status)
    assert label_of.tolist() == [0, 1, 2, 3, 4]                 # the rejected row consumes label 2
    planes = np.array([                                         # planes[z][h][w], written out by hand
        [[1, 1, 1, 0], [1, 1, 1, 0], [1, 1, 1, 0], [0, 0, 0, 0]],       # z = 0: A alone
        [[1, 1, 1, 0], [1, 3, 3, 3], [1, 3, 3, 3], [0, 3, 3, 3]],       # z = 1: B over A
        [[4, 4, 4, 4], [4, 4, 4, 4], [4, 4, 4, 4], [4, 4, 4, 4]],       # z = 2: C over both
        [[0, 0, 0, 0], [0, 3, 3, 3], [0, 3, 3, 3], [0, 3, 3, 3]],       # z = 3: B alone
    ], np.int32)
    assert seg.dtype == np.int32 and np.array_equal(np.moveaxis(seg, -1, 0), planes)
    assert 2 not in seg
    # keep drops B: the rows after it move up one label, A shows through at z = 1
    seg, label_of = S.labels(dense, status, keep=np.array([1, 1, 1, 0, 1], np.uint8))
    assert label_of.tolist() == [0, 1, 2, 0, 3]
    planes[1] = planes[0]
    planes[2] = 3
    planes[3] = 0
    assert np.array_equal(np.moveaxis(seg, -1, 0), planes)
    # nothing listed
    seg, label_of = S.labels(dense, np.full(5, U.NOT_KEPT, np.int32))
    assert not seg.any() and not label_of.any()


def test_pixelwise_counts_by_hand():
    dense, status = _cuboids()
    seg, _ = S.labels(dense, status)
    gt = np.zeros((4, 4, 4, 2), np.uint8)
    gt[:, :, 0:2, 0] = 7                                        # z = 0, 1: 32 voxels; any non-zero byte is set
    # predicted: 9 (z = 0) + 9 + 9 - 4 (z = 1) + 16 (z = 2) + 9 (z = 3) = 48 voxels, 23 of them at z < 2
    assert S.pixelwise_counts(seg, gt) == (23, 25, 9)
    assert S.pixelwise_counts(seg, gt[..., :0]) == (0, 48, 0)
    gt[0, 0, 3, 1] = 1                                          # a second mask adds one unlabelled voxel
    assert S.pixelwise_counts(seg, gt) == (23, 25, 10)
    prec, rec, f1, iou = S.pixelwise_metrics(23, 25, 9)
    assert prec == 23 / (48 + 1e-9) and rec == 23 / (32 + 1e-9) and iou == 23 / (57 + 1e-9)
    assert f1 == 2.0 * prec * rec / (prec + rec + 1e-9)
    assert abs(prec - 23 / 48) < 1e-9 and abs(f1 - 2 * 23 / (2 * 23 + 25 + 9)) < 1e-8


def test_zero_denominator_branches():
    assert S.pixelwise_metrics(0, 0, 0) == (0.0, 0.0, 0.0, 0.0)
    assert S.pixelwise_metrics(0, 5, 0) == (0.0, 0.0, 0.0, 0.0)         # tp + fn == 0: recall takes its branch
    assert S.pixelwise_metrics(0, 0, 7) == (0.0, 0.0, 0.0, 0.0)         # tp + fp == 0: precision takes its branch
    p = S.pixelwise_metrics(4, 0, 0)
    assert p == (4 / (4 + 1e-9),) * 2 + (2.0 * p[0] * p[1] / (p[0] + p[1] + 1e-9), 4 / (4 + 1e-9))
    none, some = np.zeros((2, 2, 2, 0), np.uint8), np.ones((2, 2, 2, 3), np.uint8)
    assert S.instance_dice(none, some) == (0.0, 0.0, 0) and S.instance_dice(some, none) == (0.0, 0.0, 0)
    assert S.detection_performance(none, some) == {"tp": 0, "fp": 0, "fn": 3, "recall": 0.0, "precision": 0.0}
    assert S.detection_performance(some, none) == {"tp": 0, "fp": 3, "fn": 0, "recall": 0.0, "precision": 0.0}
    assert S.detection_performance(none, none) == {"tp": 0, "fp": 0, "fn": 0, "recall": 0.0, "precision": 0.0}
    # empty masks on both sides: union 0 -> max(union, 1), IoU 0, nothing matches
    zero = np.zeros((2, 2, 2, 2), np.uint8)
    assert S.instance_dice(zero, zero) == (0.0, 0.0, 0)
    assert S.detection_performance(zero, zero) == {"tp": 0, "fp": 2, "fn": 2, "recall": 0.0, "precision": 0.0}


def _two_by_two():
    """Ten voxels in a row.  P0 = 0..5, P1 = 6..9; T0 = 0..3, T1 = 5..9:
    inter = [[4, 1], [0, 4]], IoU = [[4/6, 1/10], [0, 4/5]]."""
    pred, gt = np.zeros((1, 1, 10, 2), np.uint8), np.zeros((1, 1, 10, 2), np.uint8)
    pred[0, 0, 0:6, 0] = pred[0, 0, 6:10, 1] = 1
    gt[0, 0, 0:4, 0] = gt[0, 0, 5:10, 1] = 1
    return pred, gt


def test_matching_and_dice_by_hand():
    pred, gt = _two_by_two()
    # best pair first: (P1, T1) at 0.8, Dice 8/9; then (P0, T0) at 2/3, Dice 8/10
    dices = [2.0 * 4 / 9, 2.0 * 4 / 10]
    assert S.instance_dice(pred, gt) == (float(np.mean(dices)), float(np.std(dices)), 2)
    assert S.detection_performance(pred, gt) == {"tp": 2, "fp": 0, "fn": 0, "recall": 1.0, "precision": 1.0}
    # a bar between the two IoUs: the second pair stays unmatched
    assert S.instance_dice(pred, gt, iou_thr=0.7) == (2.0 * 4 / 9, 0.0, 1)
    assert S.detection_performance(pred, gt, thr=0.7) == {"tp": 1, "fp": 1, "fn": 1, "recall": 0.5, "precision": 0.5}
    # a used column is gone: with T1 alone P1 takes it and P0 (IoU 0.1) gets nothing
    assert S.instance_dice(pred, gt[..., 1:]) == (2.0 * 4 / 9, 0.0, 1)
    assert S.detection_performance(pred, gt[..., 1:]) == {"tp": 1, "fp": 1, "fn": 0, "recall": 1.0, "precision": 0.5}


@functools.lru_cache(maxsize=None)
def _committed():
    """U.case(8, 2) at U.SHAPE with five GT masks: three of U.case_gt, the last
    prediction itself and another one with a quarter cut away."""
    det, mask = U.case(8, 2)
    r = U.unmold(det, mask, U.SHAPE)
    gt = np.concatenate([U.case_gt(3), np.zeros(U.SHAPE + (2,), np.uint8)], -1)
    gt[..., 3] = r["dense"][U.ROWS.index("clean_otsu")]
    gt[..., 4] = r["dense"][U.ROWS.index("dense_high")]
    gt[:6, :, :, 4] = 0
    return det, r, gt


@pytest.mark.parametrize("keep_rows", [None, ("clean_otsu",), ("dense_high", "low_face_otsu")])
def test_host_functions_equal_the_restatement(keep_rows):
    from m3d import evaluate as E
    det, r, gt = _committed()
    keep = None
    if keep_rows is not None:
        keep = np.ones(len(U.ROWS), np.uint8)
        keep[[U.ROWS.index(n) for n in keep_rows]] = 0
    rows = S.listed_rows(r["status"], keep)
    masks = S.listed_masks(r["dense"], r["status"], keep)
    inter, area_gt = U.overlaps(r["dense"], gt)
    args = (inter[rows], r["area_pred"][rows], area_gt)
    want = S.instance_dice(masks, gt)
    assert E.instance_dice(*args) == want
    assert E.detection_performance(*args) == S.detection_performance(masks, gt)
    if keep_rows is None:
        assert want[2] == 2 and 0.5 < want[0] < 1.0 and want[1] > 0      # one exact match, one partial
    for thr in (0.3, 0.9):
        assert E.instance_dice(*args, iou_thr=thr) == S.instance_dice(masks, gt, thr)
        assert E.detection_performance(*args, thr=thr) == S.detection_performance(masks, gt, thr)
    seg, _ = S.labels(r["dense"], r["status"], keep)
    counts = S.pixelwise_counts(seg, gt)
    assert min(counts) > 0
    assert E.pixelwise_metrics(*counts) == S.pixelwise_metrics(*counts)
    for c in ((0, 0, 0), (0, 5, 0), (0, 0, 7), (3, 0, 0)):
        assert E.pixelwise_metrics(*c) == S.pixelwise_metrics(*c)
    for K, G in ((0, 3), (3, 0), (0, 0)):
        z = (np.zeros((K, G), np.int32), np.zeros(K, np.int32), np.zeros(G, np.int32))
        assert E.instance_dice(*z) == (0.0, 0.0, 0)
        assert E.detection_performance(*z) == S.detection_performance(np.zeros((1, 1, 1, K)), np.zeros((1, 1, 1, G)))


def test_host_functions_on_the_hand_example():
    from m3d import evaluate as E
    pred, gt = _two_by_two()
    inter, ap, ag = np.array([[4, 1], [0, 4]], np.int32), np.array([6, 4], np.int32), np.array([4, 5], np.int32)
    assert E.instance_dice(inter, ap, ag) == S.instance_dice(pred, gt)
    assert E.instance_dice(inter, ap, ag, iou_thr=0.7) == (2.0 * 4 / 9, 0.0, 1)
    assert E.detection_performance(inter, ap, ag, thr=0.7) == S.detection_performance(pred, gt, thr=0.7)
    assert E.pixelwise_metrics(23, 25, 9) == S.pixelwise_metrics(23, 25, 9)


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("shape", [(1, 5, 7), (5, 7, 3), (5, 1, 9)])
def test_imwrite_round_trips(tmp_path, dtype, shape):
    from PIL import Image
    from m3d.tiff import imread, imwrite
    rng = np.random.default_rng(shape[1])
    stack = rng.integers(0, np.iinfo(dtype).max + 1, shape).astype(dtype)
    stack[0, 0, 0], stack[-1, -1, -1] = 0, np.iinfo(dtype).max
    path = str(tmp_path / "seg.tiff")
    imwrite(path, stack)
    got = imread(path)                                          # a single page comes back as [rows, cols]
    assert got.dtype == dtype and np.array_equal(got.reshape(shape), stack)
    assert got.shape == (shape if shape[0] > 1 else shape[1:])
    with Image.open(path) as im:
        assert im.n_frames == shape[0] and im.size == (shape[2], shape[1])
        for p in range(shape[0]):
            im.seek(p)
            page = np.array(im)
            assert page.dtype == dtype and np.array_equal(page, stack[p])
    head = open(path, "rb").read(4)
    assert head == b"II*\0"                                     # little-endian baseline TIFF


def test_imwrite_rejects_what_it_cannot_write(tmp_path):
    from m3d.tiff import imwrite
    for bad in (np.zeros((2, 3), np.uint8), np.zeros((1, 2, 3), np.int32), np.zeros((1, 2, 3), np.float32),
                np.zeros((0, 2, 3), np.uint8)):
        with pytest.raises(ValueError):
            imwrite(str(tmp_path / "bad.tiff"), bad)
    # a non-contiguous view is written as the values it shows
    from m3d.tiff import imread
    a = np.arange(2 * 3 * 4, dtype=np.uint16).reshape(4, 3, 2)
    imwrite(str(tmp_path / "view.tiff"), np.moveaxis(a, -1, 0))
    assert np.array_equal(imread(str(tmp_path / "view.tiff")), np.moveaxis(a, -1, 0))


def test_csv_format(tmp_path):
    """The detection table evaluate_dataset writes beside the TIFF."""
    from m3d.evaluate import write_detection_csv
    boxes = np.array([[1.5, 0.0, 0.5, 19.2, 20.0, 15.0], [2.0, 6.3, 3.0, 22.0, 8.6, 13.0]], np.float32)
    path = str(tmp_path / "a.csv")
    write_detection_csv(path, np.array([2, 1], np.int32), boxes)
    lines = open(path, newline="").read().splitlines()
    assert lines[0] == "class,y1,x1,z1,y2,x2,z2" and len(lines) == 3
    assert lines[1] == "2,1.5,0.0,0.5,19.2,20.0,15.0"
    got = list(csv.reader(lines[1:]))
    assert [int(r[0]) for r in got] == [2, 1]
    assert np.array_equal(np.array([r[1:] for r in got], np.float32), boxes)    # float32 text round-trips
    write_detection_csv(path, np.zeros(0, np.int32), np.zeros((0, 6), np.float32))
    assert open(path, newline="").read().splitlines() == ["class,y1,x1,z1,y2,x2,z2"]
