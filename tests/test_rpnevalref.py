"""tests/rpnevalref.py (the restatement of the reference's per-image RPN scoring)
and m3d.rpn_eval.summarize against answers worked out by hand.  Every box sits
on a grid of 8 voxels, so the normalised proposals (pixels / 8) and every IoU
below are exact in float32."""
import math

import numpy as np

import rpnevalref as E

SHAPE = (8, 8, 8)
NONE = 2 ** 31 - 1


def _rois(*px):
    return (np.array(px, np.float32).reshape(-1, 6) / np.float32(8)).astype(np.float32)


def _score(rois, gt, topk=10, match_iou=0.5, grid=(0.5,)):
    return E.score(rois, np.array(gt, np.float32).reshape(-1, 6), SHAPE, topk, match_iou, list(grid))


def test_iou_on_the_threshold_is_a_hit_but_not_a_match():
    """inter 4, union 8 + 4 - 4 = 8: IoU exactly 0.5.  `>` rejects it, `>=` takes it."""
    r = _score(_rois((0, 0, 0, 2, 2, 1)), [(0, 0, 0, 2, 2, 2)])
    assert r["iou"].tobytes() == np.array([[0.5]], np.float32).tobytes()
    assert r["assoc"].tolist() == [-1] and not r["matched"].any()
    assert r["first_hit"].tolist() == [[0]] and r["counts"].tolist() == [1, 0]
    # a threshold one float64 step under 0.5 matches: the compare is in double
    r = _score(_rois((0, 0, 0, 2, 2, 1)), [(0, 0, 0, 2, 2, 2)], match_iou=math.nextafter(0.5, 0.0))
    assert r["assoc"].tolist() == [0] and r["matched"].tolist() == [[0, 0, 0, 2, 2, 1]]
    # ... and a grid threshold that rounds to 0.5 in float32 still hits, one that does not, does not
    assert _score(_rois((0, 0, 0, 2, 2, 1)), [(0, 0, 0, 2, 2, 2)], grid=(0.5 + 1e-9,))["first_hit"].tolist() == [[0]]
    assert _score(_rois((0, 0, 0, 2, 2, 1)), [(0, 0, 0, 2, 2, 2)], grid=(0.5 + 1e-7,))["first_hit"].tolist() == [[NONE]]


def test_two_identical_gt_boxes_the_first_takes_the_roi():
    r = _score(_rois((0, 0, 0, 4, 4, 4)), [(0, 0, 0, 4, 4, 4), (0, 0, 0, 4, 4, 4)])
    assert r["assoc"].tolist() == [0, -1]
    assert r["matched"].tolist() == [[0, 0, 0, 4, 4, 4], [0] * 6]
    assert r["first_hit"].tolist() == [[0, 0]]              # the grid knows no claims: both are hit


def test_a_later_better_roi_does_not_displace_a_claim():
    r = _score(_rois((0, 0, 0, 4, 4, 3), (0, 0, 0, 4, 4, 4)), [(0, 0, 0, 4, 4, 4)], grid=(0.5, 0.8))
    assert r["iou"].tolist() == [[0.75, 1.0]]
    assert r["assoc"].tolist() == [0] and r["matched"].tolist() == [[0, 0, 0, 4, 4, 3]]
    assert r["first_hit"].tolist() == [[0], [1]]
    # a ROI under the threshold claims nothing: the later one does
    r = _score(_rois((0, 0, 0, 4, 4, 1), (0, 0, 0, 4, 4, 4)), [(0, 0, 0, 4, 4, 4)])
    assert r["iou"].tolist() == [[0.25, 1.0]] and r["assoc"].tolist() == [1]
    # topk cuts the walk, not the grid
    r = _score(_rois((0, 0, 0, 4, 4, 1), (0, 0, 0, 4, 4, 4)), [(0, 0, 0, 4, 4, 4)], topk=1)
    assert r["assoc"].tolist() == [-1] and r["first_hit"].tolist() == [[1]] and r["counts"].tolist() == [1, 0]


def test_a_zero_padded_row_is_the_unit_box():
    px, valid = E.pixel_boxes(np.zeros((2, 6), np.float32), SHAPE)
    assert valid.tolist() == [True, True] and px.tolist() == [[0, 0, 0, 1, 1, 1]] * 2
    r = _score(np.zeros((2, 6), np.float32), [(0, 0, 0, 1, 1, 2)])
    assert r["iou"].tolist() == [[0.5, 0.5]] and r["assoc"].tolist() == [-1] and r["counts"].tolist() == [2, 0]
    r = _score(np.zeros((2, 6), np.float32), [(0, 0, 0, 1, 1, 1)])
    assert r["assoc"].tolist() == [0] and r["matched"].tolist() == [[0, 0, 0, 1, 1, 1]]


def test_invalid_rows_nan_flat_and_out_of_range():
    rois = _rois((4, 0, 0, 2, 8, 8), (0, 0, 0, 0, 0, 0), (-3, -3, -3, 12, 12, 12), (2, 2, 2, 2, 4, 4))
    rois[1, 2] = np.nan
    px, valid = E.pixel_boxes(rois, SHAPE)
    assert valid.tolist() == [False, False, True, False]
    assert px[2].tolist() == [0, 0, 0, 8, 8, 8]             # clamped to the volume
    r = _score(rois, [(0, 0, 0, 8, 8, 8)])
    assert r["iou"].tolist() == [[0, 0, 1, 0]] and r["assoc"].tolist() == [2] and r["counts"].tolist() == [1, 2]
    assert _score(rois[:2], [(0, 0, 0, 8, 8, 8)])["counts"].tolist() == [0, NONE]
    empty = _score(np.zeros((0, 6), np.float32), [(0, 0, 0, 8, 8, 8)])
    assert empty["counts"].tolist() == [0, NONE] and empty["assoc"].tolist() == [-1] and empty["iou"].shape == (1, 0)


def test_a_gt_box_with_swapped_corners_scores_as_its_normalised_form():
    rois = _rois((0, 0, 0, 2, 2, 1), (1, 1, 1, 3, 3, 3))
    a, b = _score(rois, [(2, 2, 2, 0, 0, 0)]), _score(rois, [(0, 0, 0, 2, 2, 2)])
    assert a["iou"].tobytes() == b["iou"].tobytes() and a["iou"].tolist() == [[0.5, float(np.float32(1) / np.float32(15))]]
    assert a["assoc"].tolist() == b["assoc"].tolist() == [-1]


def _summary(records, cl, bl, gts, topk_grid=(1, 2), grid=(0.5, 0.8)):
    from m3d.rpn_eval import summarize
    return summarize(records, cl, bl, gts, list(topk_grid), list(grid))


def test_a_prefix_shorter_than_the_first_valid_row_is_skipped():
    gt = np.array([(0, 0, 0, 4, 4, 4)], np.float32)
    r = _score(_rois((4, 0, 0, 2, 8, 8), (0, 0, 0, 4, 4, 4)), gt, grid=(0.5, 0.8))
    assert r["counts"].tolist() == [1, 1] and r["first_hit"].tolist() == [[1], [1]]
    s = _summary([r], [1.0], [2.0], [gt])
    assert s["detection_at"] == {"0.50@2": 100.0, "0.80@2": 100.0}          # no "@1" key at all
    assert s["rpn_test_detection_score"] == 100.0 and s["rpn_test_mean_coord_error"] == 0.0


def test_summarize_branches_means_and_stds():
    nan_row = np.full((1, 6), np.nan, np.float32)
    two = _rois((0, 0, 0, 4, 4, 3), (0, 0, 0, 4, 4, 4))
    gt_b = np.array([(0, 0, 0, 8, 8, 8)], np.float32)
    gt_c = np.array([(4, 4, 4, 8, 8, 8)], np.float32)
    gt_d = np.array([(0, 0, 0, 4, 4, 4), (4, 4, 4, 8, 8, 8)], np.float32)
    rec_b = _score(nan_row, gt_b, grid=(0.5, 0.8))           # no valid ROI: losses only
    rec_c = _score(two, gt_c, grid=(0.5, 0.8))               # valid ROIs, nothing matched: score 0, grid counted
    rec_d = _score(two, gt_d, grid=(0.5, 0.8))               # g0 claimed by row 0 (IoU 0.75), g1 by nothing
    assert rec_b["counts"].tolist() == [0, NONE]
    assert rec_c["assoc"].tolist() == [-1] and rec_d["assoc"].tolist() == [0, -1]
    s = _summary([None, rec_b, rec_c, rec_d], [1.0, 2.0, 3.0, 6.0], [0.5, 0.5, 0.5, 0.5],
                 [np.zeros((0, 6), np.float32), gt_b, gt_c, gt_d])
    assert s["rpn_test_class_mean"] == 3.0 and s["rpn_test_class_std"] == math.sqrt(3.5)
    assert s["rpn_test_bbox_mean"] == 0.5 and s["rpn_test_bbox_std"] == 0.0
    assert s["rpn_test_detection_score"] == 25.0             # mean(0, 50)
    assert s["rpn_test_mean_coord_error"] == 1.0 / 6.0       # |(0,0,0,4,4,3) - (0,0,0,4,4,4)|, image d alone
    assert s["detection_at"] == {"0.50@1": 25.0, "0.80@1": 0.0, "0.50@2": 25.0, "0.80@2": 25.0}
    assert set(s) == {"rpn_test_class_mean", "rpn_test_class_std", "rpn_test_bbox_mean", "rpn_test_bbox_std",
                      "rpn_test_mean_coord_error", "rpn_test_detection_score", "detection_at"}
    # the packed int32 row gives the same numbers as the dict
    from m3d.rpn_eval import record_len, unpack_record
    row = np.concatenate([rec_d["counts"], rec_d["assoc"], rec_d["matched"].reshape(-1).view(np.int32),
                          rec_d["first_hit"].reshape(-1), np.zeros(5, np.int32)])
    assert record_len(2, 2) == len(row) - 5
    u = unpack_record(row, 2, 2)
    assert all(np.array_equal(u[k], rec_d[k]) for k in ("counts", "assoc", "matched", "first_hit"))
    assert _summary([None, rec_b, rec_c, row], [1.0, 2.0, 3.0, 6.0], [0.5] * 4,
                    [None, gt_b, gt_c, gt_d]) == s


def test_summarize_empty_defaults():
    s = _summary([], [], [], [])
    assert s["detection_at"] == {} and all(v == 0.0 for k, v in s.items() if k != "detection_at")
    # only images without GT: the losses count, everything else stays at its zero default
    s = _summary([None, None], [1.0, 3.0], [2.0, 2.0], [np.zeros((0, 6), np.float32)] * 2)
    assert (s["rpn_test_class_mean"], s["rpn_test_class_std"], s["rpn_test_bbox_mean"]) == (2.0, 1.0, 2.0)
    assert s["rpn_test_detection_score"] == 0.0 and s["rpn_test_mean_coord_error"] == 0.0 and s["detection_at"] == {}
    from m3d.rpn_eval import summarize
    assert "rpn_train_class_mean" in summarize([], [], [], [], [1], [0.5], subset="train")
