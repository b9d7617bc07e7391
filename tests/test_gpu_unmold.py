"""Detection unmolding and mask-IoU evaluation on the GPU (csrc/unmold.hip,
m3d.evaluate) against the numpy float64 restatement tests/unmoldref.py (pinned
by tests/test_unmoldref.py).

Bars: small, box_i, status, area_pred, inter, area_gt, dense and seg_union are
integers and equal the restatement bit for bit; so do thr / resize_thr (chosen
from exact order statistics and an exactly ordered Otsu scan) and the float32
IoU.  min / max / p50 / p95 come from the sorted values (exact); mean and std
are fp64 sums of <= 32768 terms in another order than numpy's: 1e-10 relative
leaves 25x over the 4e-12 such a reassociation can move them.

Shapes: volume 24 x 20 x 16, twelve detections (tests/unmoldref.py ROWS: one
row per status code, threshold branch and box edge case), m = 28 (the real
LDS footprint and sort size) and m = 8, C = 2 and 1, G = 1, 3, 17 and 1030
(more GT bytes per voxel than one pass of the workgroup takes: 1024); one case
at 128 x 128 x 64 with G = 40 for many slabs per detection, and one with G =
4200 there, whose GT volume is 4.4 GB, so that byte offsets pass 2^31 and 2^32."""
import functools

import numpy as np
import pytest
import torch

import unmoldref as U

pytestmark = pytest.mark.gpu

SHAPE = U.SHAPE


@functools.lru_cache(maxsize=None)
def _ref(m, C):
    det, mask = U.case(m, C)
    return det, mask, U.unmold(det, mask, SHAPE)


@functools.lru_cache(maxsize=None)
def _ref_overlaps(m, C, G):
    r = _ref(m, C)[2]
    gt = U.case_gt(G)
    inter, area_gt = U.overlaps(r["dense"], gt)
    return gt, inter, area_gt, U.iou_matrix(inter, r["area_pred"], area_gt)


def _np(t):
    return t.cpu().numpy()


def _same_f32(got, want):
    """Bit-equal float32 arrays; NaNs at the same places (their payload is not compared)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[~nan].view(np.int32), want[~nan].view(np.int32))


def _check_unmolded(u, r, dense=True):
    assert np.array_equal(_np(u.status), r["status"]), (_np(u.status), r["status"])
    assert np.array_equal(_np(u.box_i), r["box_i"])
    assert np.array_equal(_np(u.small), r["small"])
    assert np.array_equal(_np(u.area_pred), r["area_pred"])
    st, want = _np(u.stats), r["stats"]
    print("stats max relative difference", np.abs(st - want).max() / max(np.abs(want).max(), 1e-300))
    assert np.array_equal(st[:, 6:], want[:, 6:])                # thr, resize_thr: bit-equal
    assert np.array_equal(st[:, [0, 1, 4, 5]], want[:, [0, 1, 4, 5]])   # order statistics: exact
    assert np.all(np.abs(st[:, 2:4] - want[:, 2:4]) <= 1e-10 * np.abs(want[:, 2:4]) + 1e-300)
    if dense:
        assert np.array_equal(_np(u.dense), r["dense"])
        assert np.array_equal(_np(u.seg_union), r["seg_union"])
        assert u.masks.shape == SHAPE + (len(r["status"]),)
        assert torch.equal(u.masks[..., 2], u.dense[2])


@pytest.mark.parametrize("m,C", [(28, 2), (8, 2), (8, 1)])
def test_unmold_equals_the_restatement(cuda, m, C):
    from m3d import evaluate as E
    det, mask, r = _ref(m, C)
    u = E.unmold_detections(torch.from_numpy(det).to(cuda), torch.from_numpy(mask).to(cuda), SHAPE, dense=True,
                            union=True)
    _check_unmolded(u, r)
    with pytest.raises(ValueError, match="logits"):
        u.compact()                                             # the RANGE row
    keep = [i for i, n in enumerate(U.ROWS) if n != "range"]
    u2 = E.unmold_detections(torch.from_numpy(det[keep]).to(cuda), torch.from_numpy(mask[keep]).to(cuda), SHAPE)
    assert u2.dense is None and u2.seg_union is None and u2.masks is None
    k = u2.compact()
    boxes, scores, ids, rows = U.compact(det[keep], r["status"][keep], SHAPE)
    assert np.array_equal(k["boxes"], boxes) and np.array_equal(k["scores"], scores)
    assert np.array_equal(k["class_ids"], ids) and np.array_equal(k["rows"], rows)
    assert np.array_equal(k["status"], r["status"][keep][rows]) and np.array_equal(k["area"], r["area_pred"][keep][rows])


@pytest.mark.parametrize("m,C,G", [(8, 2, 1), (8, 2, 3), (8, 1, 17), (28, 2, 17), (8, 2, 1030)])
def test_overlaps_equal_the_restatement(cuda, m, C, G):
    from m3d import evaluate as E
    det, mask, r = _ref(m, C)
    gt, inter, area_gt, iou = _ref_overlaps(m, C, G)
    u = E.unmold_detections(torch.from_numpy(det).to(cuda), torch.from_numpy(mask).to(cuda), SHAPE)
    got = E.mask_overlaps(u, torch.from_numpy(gt).to(cuda))
    assert np.array_equal(_np(got[1]), inter) and np.array_equal(_np(got[2]), r["area_pred"])
    assert np.array_equal(_np(got[3]), area_gt)
    assert np.array_equal(_np(E.mask_areas(torch.from_numpy(gt).to(cuda))), area_gt)
    _same_f32(_np(got[0]), iou)
    assert inter.any()
    if G > 1:                                                   # the all-zero GT mask against the empty predictions
        assert area_gt[-1] == 0 and np.isnan(iou[r["area_pred"] == 0, -1]).all() and np.isnan(iou[:, -1]).any()
        assert (np.count_nonzero(inter, axis=1) > 1).any()      # overlapping GT masks: one voxel counted for several
    # the GT masks given to unmold_detections: the same results from its one traversal
    u1 = E.unmold_detections(torch.from_numpy(det).to(cuda), torch.from_numpy(mask).to(cuda), SHAPE,
                             gt_masks=torch.from_numpy(gt).to(cuda))
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got, u1.overlaps))
    assert torch.equal(u1.area_pred, u.area_pred) and torch.equal(u1.status, u.status) and u.overlaps is None
    # bool GT masks are read in place
    got_b = E.mask_overlaps(u, torch.from_numpy(gt.astype(bool)).to(cuda))
    assert all(torch.equal(a, b) or (a.is_floating_point() and torch.equal(a.isnan(), b.isnan()))
               for a, b in zip(got, got_b))


def _raw(cuda, det, mask, gt, shape, dense=None, union=None, iou=None, inter=None):
    """The launch sequence through the C-ABI on caller-made outputs."""
    import m3d._lib as lib
    L, p, s = lib.load(), lib.ptr, lib.stream()
    n, m, C = det.shape[0], mask.shape[1], mask.shape[-1]
    H, W, D = shape
    G = 0 if gt is None else gt.shape[-1]
    o = {"small": torch.empty((n, m ** 3), dtype=torch.uint8, device=cuda),
         "box_i": torch.empty((n, 6), dtype=torch.int32, device=cuda),
         "status": torch.empty(n, dtype=torch.int32, device=cuda),
         "stats": torch.empty((n, 8), dtype=torch.float64, device=cuda),
         "area_pred": torch.empty(n, dtype=torch.int32, device=cuda),
         "inter": inter if inter is not None else torch.empty((n, max(G, 1)), dtype=torch.int32, device=cuda),
         "area_gt": torch.empty(max(G, 1), dtype=torch.int32, device=cuda), "iou": iou, "dense": dense,
         "seg_union": union}
    lib.check(L.m3d_unmold_prepare(p(det), p(mask), n, m, C, H, W, D, p(o["small"]), p(o["box_i"]), p(o["status"]),
                                   p(o["stats"]), s))
    lib.check(L.m3d_unmold_overlaps(p(o["small"]), p(o["box_i"]), p(o["status"]), p(o["stats"]), n, m, H, W, D,
                                    p(gt), G, p(o["area_pred"]), p(o["inter"]), s))
    if G:
        lib.check(L.m3d_mask_areas(p(gt), H, W, D, G, p(o["area_gt"]), s))
    lib.check(L.m3d_unmold_finalize(p(o["box_i"]), p(o["status"]), n, G, p(o["area_pred"]),
                                    p(o["inter"]), p(o["area_gt"]), p(iou), s))
    if dense is not None or union is not None:
        lib.check(L.m3d_unmold_paste(p(o["small"]), p(o["box_i"]), p(o["status"]), p(o["stats"]), n, m, H, W, D,
                                     p(dense), p(union), s))
    return o


def test_two_runs_are_bit_identical(cuda):
    det, mask, r = _ref(28, 2)
    gt = torch.from_numpy(_ref_overlaps(28, 2, 17)[0]).to(cuda)
    d, k = torch.from_numpy(det).to(cuda), torch.from_numpy(mask).to(cuda)
    runs = []
    for _ in range(2):
        n = det.shape[0]
        runs.append(_raw(cuda, d, k, gt, SHAPE, dense=torch.zeros((n,) + SHAPE, dtype=torch.uint8, device=cuda),
                         union=torch.zeros(SHAPE, dtype=torch.uint8, device=cuda),
                         iou=torch.empty((n, 17), dtype=torch.float32, device=cuda)))
    torch.cuda.synchronize()
    for key in runs[0]:
        a, b = runs[0][key], runs[1][key]
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), key    # bytes: NaNs included


def test_outputs_not_requested_stay_untouched(cuda):
    """Poisoned buffers: the paste stores nothing but the 1s of set voxels; with
    G = 0 neither inter nor iou is written; each of dense / seg_union alone."""
    det, mask, r = _ref(8, 2)
    d, k = torch.from_numpy(det).to(cuda), torch.from_numpy(mask).to(cuda)
    n = det.shape[0]
    dense = torch.full((n,) + SHAPE, 0xFF, dtype=torch.uint8, device=cuda)
    union = torch.full(SHAPE, 0xFF, dtype=torch.uint8, device=cuda)
    inter = torch.full((n, 5), -7, dtype=torch.int32, device=cuda)
    iou = torch.full((n, 5), float("nan"), dtype=torch.float32, device=cuda)
    o = _raw(cuda, d, k, None, SHAPE, dense=dense, union=union, iou=iou, inter=inter)
    assert np.array_equal(_np(dense), np.where(r["dense"] == 1, 1, 0xFF))
    assert np.array_equal(_np(union), np.where(r["seg_union"] == 1, 1, 0xFF))
    assert (inter == -7).all() and iou.isnan().all()
    assert np.array_equal(_np(o["area_pred"]), r["area_pred"]) and np.array_equal(_np(o["status"]), r["status"])
    # finalize without iou on G > 0 leaves a poisoned iou alone; one paste target at a time
    gt, want_inter, _, _ = _ref_overlaps(8, 2, 3)
    dense.fill_(0)
    union.fill_(0xFF)
    o = _raw(cuda, d, k, torch.from_numpy(gt).to(cuda), SHAPE, dense=dense, union=None, iou=None)
    assert np.array_equal(_np(o["inter"]), want_inter) and np.array_equal(_np(dense), r["dense"])
    assert (union == 0xFF).all() and iou.isnan().all()
    dense.fill_(0xFF)
    union.fill_(0)
    _raw(cuda, d, k, None, SHAPE, dense=None, union=union)
    assert np.array_equal(_np(union), r["seg_union"]) and (dense == 0xFF).all()


def test_graph_capture_and_replay(cuda):
    """unmold (dense + union) and the overlaps captured in one HIP graph on one
    stream, replayed on poisoned outputs: bit-equal to the restatement."""
    from m3d import evaluate as E
    det, mask, r = _ref(28, 2)
    gt_h, inter, area_gt, iou = _ref_overlaps(28, 2, 17)
    d, k, gt = torch.from_numpy(det).to(cuda), torch.from_numpy(mask).to(cuda), torch.from_numpy(gt_h).to(cuda)

    def run():
        u = E.unmold_detections(d, k, SHAPE, dense=True, union=True)
        return u, E.mask_overlaps(u, gt)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        u, ov = run()
    for t in (u.small, u.dense, u.seg_union):
        t.fill_(0xFF)
    for t in (u.status, u.box_i, u.area_pred, ov[1], ov[2], ov[3]):
        t.fill_(-1)
    ov[0].fill_(float("nan"))
    u.stats.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    _check_unmolded(u, r)
    assert np.array_equal(_np(ov[1]), inter) and np.array_equal(_np(ov[2]), r["area_pred"])
    assert np.array_equal(_np(ov[3]), area_gt)
    _same_f32(_np(ov[0]), iou)


def test_many_slabs_per_detection(cuda):
    """128 x 128 x 64, G = 40, m = 28: a box over most of the volume (64 slabs,
    several sweeps each), one mid-sized box, one padding row."""
    from m3d import evaluate as E
    shape = (128, 128, 64)
    grids = U.case_grids(28, seed=3)
    det = np.zeros((3, 8), np.float32)
    det[0] = [0.02, 0.01, 0.03, 0.97, 0.99, 0.96, 1, 0.9]
    det[1] = [0.30, 0.25, 0.10, 0.62, 0.70, 0.55, 1, 0.8]
    mask = np.zeros((3, 28, 28, 28, 2), np.float32)
    mask[0, ..., 1], mask[1, ..., 1] = grids["clean_otsu"], grids["low_face_otsu"]
    r = U.unmold(det, mask, shape)
    assert r["status"].tolist() == [U.OK, U.OK, U.NOT_KEPT] and r["area_pred"][0] > 100000
    gt = U.case_gt(40, shape, seed=1)
    inter, area_gt = U.overlaps(r["dense"], gt)
    u = E.unmold_detections(torch.from_numpy(det).to(cuda), torch.from_numpy(mask).to(cuda), shape, dense=True,
                            union=True)
    got = E.mask_overlaps(u, torch.from_numpy(gt).to(cuda))
    assert np.array_equal(_np(u.area_pred), r["area_pred"]) and np.array_equal(_np(u.status), r["status"])
    assert np.array_equal(_np(got[1]), inter) and np.array_equal(_np(got[3]), area_gt)
    _same_f32(_np(got[0]), U.iou_matrix(inter, r["area_pred"], area_gt))
    assert np.array_equal(_np(u.dense), r["dense"]) and np.array_equal(_np(u.seg_union), r["seg_union"])


def test_gt_offsets_past_32_bits(cuda):
    """128 x 128 x 64 with G = 4200: the GT volume is 4.4 GB.  A voxel's GT row
    starts at byte lin * G, past 2^31 from y = 63 on and past 2^32 from y = 125
    on; the box spans y = 70..126.  Ten GT masks are set -- the first and last
    column of each 1024-byte pass -- each over its own part of the box, the
    rest are zero; built on the device, never on the host.  A truncated offset
    reads other columns or other voxels."""
    from m3d import evaluate as E
    shape, G = (128, 128, 64), 4200
    cols = [0, 1023, 1024, 2047, 2048, 3071, 3072, 4095, 4096, 4199]
    det = np.zeros((2, 8), np.float32)
    det[0] = [0.55, 0.2, 0.1, 0.99, 0.8, 0.9, 1, 0.9]
    mask = np.zeros((2, 28, 28, 28, 2), np.float32)
    mask[0, ..., 1] = U.case_grids(28, seed=3)["clean_otsu"]
    r = U.unmold(det, mask, shape)
    assert r["status"].tolist() == [U.OK, U.NOT_KEPT] and r["box_i"][0, 0] == 70 and r["box_i"][0, 3] == 127
    assert (70 * 128 * 64) * G > 2 ** 31 and (126 * 128 * 64 + 25 * 64) * G > 2 ** 32
    gt_cols = U.case_gt(len(cols) + 1, shape, seed=2)[..., :len(cols)]          # (its last mask is the empty one)
    for k in range(len(cols)):
        gt_cols[72 + 5 * k:80 + 5 * k, :, :, k] = 1                             # each meets its own part of the box
    gt_cols[60:, :, :, 3] = 1                                                   # and one covers it whole
    inter_c, area_c = U.overlaps(r["dense"], gt_cols)
    inter, area_gt = np.zeros((2, G), np.int32), np.zeros(G, np.int32)
    inter[:, cols], area_gt[cols] = inter_c, area_c
    assert inter_c[0].min() > 0 and inter_c[0, 3] == r["area_pred"][0] and len(set(inter_c[0].tolist())) == len(cols)
    gt = torch.zeros(shape + (G,), dtype=torch.uint8, device=cuda)
    gt[..., torch.tensor(cols, device=cuda)] = torch.from_numpy(gt_cols).to(cuda)
    u = E.unmold_detections(torch.from_numpy(det).to(cuda), torch.from_numpy(mask).to(cuda), shape, gt_masks=gt)
    iou, got_inter, got_area, got_area_gt = u.overlaps
    assert np.array_equal(_np(got_area), r["area_pred"])
    assert np.array_equal(_np(got_area_gt), area_gt) and np.array_equal(_np(got_inter), inter)
    _same_f32(_np(iou), U.iou_matrix(inter, r["area_pred"], area_gt))


def test_maskrcnn_evaluate_end_to_end(cuda):
    """MaskRCNN.evaluate on the toy 64^3 config, random weights, fixed seed: its
    IoU / AP equal the restatement fed with detect's own outputs; with the GT
    masks replaced by the unmolded prediction masks the AP over the detections
    that have a mask is exactly 1."""
    from m3d import evaluate as E
    from m3d.config import synthetic_mrcnn_config
    from m3d.heads import MaskRCNN
    from m3d.model import compose_image_meta, synthetic_volume
    S = 64
    cfg = synthetic_mrcnn_config(S, PRE_NMS_LIMIT=2000, POST_NMS_ROIS_INFERENCE=64, DETECTION_MAX_INSTANCES=8,
                                 DETECTION_MIN_CONFIDENCE=0.0, MASK_SHAPE=[28, 28, 28])
    model = MaskRCNN(cfg, device=cuda, seed=2)
    meta = torch.from_numpy(compose_image_meta(0, [S, S, S, 1], [S, S, S, 1], [0, 0, 0, S, S, S], 1.0,
                                               [1, 1])[None]).to(cuda)
    image = synthetic_volume(S).to(cuda)
    boxes = np.array([[4, 4, 8, 32, 36, 40], [30, 8, 20, 60, 34, 60], [12, 36, 0, 40, 62, 30]], np.float32)
    gt = np.zeros((S, S, S, 3), np.uint8)
    for g, (y1, x1, z1, y2, x2, z2) in enumerate(boxes.astype(int)):
        gt[y1:y2, x1:x2, z1:z2, g] = 1
    gt_ids = np.ones(3, np.int32)
    out = model.evaluate(image, meta, torch.from_numpy(gt_ids).to(cuda), torch.from_numpy(boxes[None]).to(cuda),
                         torch.from_numpy(gt).to(cuda))
    det, mask = _np(out["detections"][0]), _np(out["mrcnn_mask"][0])
    r = U.unmold(det, mask, (S, S, S))
    print("status", r["status"].tolist(), "area", r["area_pred"].tolist(), "mAP", out["mAP"])
    u = out["unmolded"]
    assert np.array_equal(_np(u.status), r["status"]) and np.array_equal(_np(u.area_pred), r["area_pred"])
    assert np.array_equal(_np(u.small), r["small"]) and np.array_equal(_np(u.box_i), r["box_i"])
    inter, area_gt = U.overlaps(r["dense"], gt)
    _, _, ids, rows = U.compact(det, r["status"], (S, S, S))
    iou = U.iou_matrix(inter, r["area_pred"], area_gt)[rows]
    _same_f32(out["iou"], iou)
    assert np.array_equal(out["inter"], inter[rows]) and np.array_equal(out["rows"], rows)
    want = U.compute_ap(iou, ids, gt_ids)
    assert (out["mAP"], out["precision"], out["recall"]) == want[:3]
    assert np.array_equal(np.array(out["ious"]), np.array(want[3]), equal_nan=True)
    # the prediction masks as ground truth
    ok = np.flatnonzero(r["status"] == U.OK)
    assert len(ok) > 0, "no detection of the random-weight model kept a mask"
    u = E.unmold_detections(out["detections"][0], out["mrcnn_mask"][0], (S, S, S), dense=True)
    gt2 = u.masks[..., torch.from_numpy(ok).to(cuda)].contiguous()
    out2 = E.evaluate_detections(out["detections"][0], out["mrcnn_mask"][0], (S, S, S), det[ok, 6].astype(np.int32),
                                 gt2)
    sel = np.flatnonzero(np.isin(out2["rows"], ok))
    assert np.array_equal(np.diagonal(out2["iou"][sel]), np.ones(len(ok), np.float32))
    mAP, precision, recall, ious = E.compute_ap(out2["iou"][sel], out2["class_ids"][sel], det[ok, 6].astype(np.int32))
    assert (mAP, precision, recall) == (1.0, 1.0, 1.0) and len(ious) == len(ok)
    if len(ok) == len(out2["rows"]):
        assert out2["mAP"] == 1.0
