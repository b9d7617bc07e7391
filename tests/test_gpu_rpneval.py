"""m3d_rpn_eval_proposals / m3d.rpn_eval / RPN.evaluate on the GPU.  Every
output of the kernel -- assoc, matched, first_hit, counts and the optional IoU
matrix -- is compared bit for bit with the NumPy restatement tests/rpnevalref.py:
the IoU is a fixed sequence of float32 operations and everything that crosses
threads is an integer minimum or count, so there is no tolerance to set.

The scoring kernel takes CHUNK = 256 proposals per workgroup (one per thread,
four waves); the sizes below cross every lane, wave and workgroup boundary
(1, 63, 65, 255, 256, 257, 1025, 8000)."""
import bz2
import csv
import os
import pickle

import numpy as np
import pytest
import torch

import rpnevalref as E

pytestmark = pytest.mark.gpu

CHUNK = 256
PAD = 64                   # guard words around every output
GUARD = 0x5A5A5A5A
SHAPE = (64, 48, 20)
GRID3 = [0.30, 0.40, 0.50]


def _guarded(cuda, n):
    buf = torch.full((PAD + n + PAD,), GUARD, dtype=torch.int32, device=cuda)
    return buf, buf[PAD:PAD + n]


def _gpu(cuda, rois, gt, shape, topk, thr, grid, want_iou=True):
    """The raw entry point with guard bands around every output -> dict of host arrays."""
    import m3d._lib as lib
    L, p = lib.load(), lib.ptr
    R, G, T = len(rois), len(gt), len(grid)
    d_rois = torch.from_numpy(np.ascontiguousarray(rois, np.float32)).to(cuda)
    d_gt = torch.from_numpy(np.ascontiguousarray(gt, np.float32)).to(cuda)
    d_grid = torch.tensor([float(v) for v in grid], dtype=torch.float32, device=cuda)
    sizes = {"assoc": G, "matched": 6 * G, "first_hit": T * G, "counts": 2, "iou": G * R if want_iou else 0}
    bufs = {k: _guarded(cuda, n) for k, n in sizes.items()}
    o = {k: v[1] for k, v in bufs.items()}
    H, W, D = shape
    lib.check(L.m3d_rpn_eval_proposals(p(d_rois) if R else None, R, p(d_gt), G, H, W, D, topk, thr,
                                       p(d_grid) if T else None, T, p(o["assoc"]), p(o["matched"]),
                                       p(o["first_hit"]) if T else None, p(o["counts"]),
                                       p(o["iou"]) if want_iou and R else None, lib.stream()), "m3d_rpn_eval_proposals")
    torch.cuda.synchronize()
    for k, (buf, _) in bufs.items():
        host = buf.cpu().numpy()
        assert (host[:PAD] == GUARD).all() and (host[PAD + sizes[k]:] == GUARD).all(), f"guard band of {k} overwritten"
    out = {k: o[k].cpu().numpy() for k in ("assoc", "first_hit", "counts")}
    out["first_hit"] = out["first_hit"].reshape(T, G)
    out["matched"] = o["matched"].cpu().numpy().view(np.float32).reshape(G, 6)
    if want_iou:
        out["iou"] = o["iou"].cpu().numpy().view(np.float32).reshape(G, R)
    return out


def _assert_same(got, want, what=""):
    for k in got:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k)
        if got[k].tobytes() != want[k].tobytes():
            bad = np.argwhere(got[k].view(np.int32) != want[k].view(np.int32))
            raise AssertionError(f"{what} {k}: {len(bad)} of {got[k].size} differ, first at {bad[0].tolist()}: "
                                 f"gpu {got[k][tuple(bad[0])]!r} ref {want[k][tuple(bad[0])]!r}")


def _check(cuda, rois, gt, shape=SHAPE, topk=512, thr=0.5, grid=GRID3, what=""):
    want = E.score(rois, gt, shape, topk, thr, grid)
    _assert_same(_gpu(cuda, rois, gt, shape, topk, thr, grid), want, what)
    return want


def _case(seed, R, G, shape=SHAPE, near=0.5, padded=0.1, spread=3.0):
    """G GT boxes at non-integer pixel coordinates and R normalised proposals:
    `near` of them a GT box shifted by sub-voxel or few-voxel offsets (so the
    IoUs straddle the thresholds and an fma would change their bits), `padded`
    of them zero rows, the rest uniform random boxes; in a random order."""
    rng = np.random.default_rng(seed)
    dims = np.array(shape, np.float64)
    lo = rng.uniform(0.0, 0.65, (G, 3)) * dims
    gt = np.concatenate([lo, lo + rng.uniform(0.08, 0.3, (G, 3)) * dims], 1).astype(np.float32)
    kind = rng.uniform(size=R)
    which = rng.integers(0, G, R)
    scale = np.where(rng.uniform(size=(R, 1)) < 0.5, 0.4, spread)
    px_near = gt[which].astype(np.float64) + rng.normal(size=(R, 6)) * scale
    a, b = rng.uniform(0.0, 1.0, (R, 3)) * dims, rng.uniform(0.0, 1.0, (R, 3)) * dims
    px_rand = np.concatenate([np.minimum(a, b), np.maximum(a, b)], 1)
    px = np.where((kind < near)[:, None], px_near, px_rand)
    rois = (px / np.concatenate([dims, dims])).astype(np.float32)
    rois[kind > 1.0 - padded] = 0.0
    return rois, gt


def _px8(*boxes):
    return (np.array(boxes, np.float32).reshape(-1, 6) / np.float32(8)).astype(np.float32)


def test_hand_cases(cuda):
    s8 = (8, 8, 8)
    one = np.array([(0, 0, 0, 2, 2, 2)], np.float32)
    w = _check(cuda, _px8((0, 0, 0, 2, 2, 1)), one, s8, 10, 0.5, [0.5], "threshold")
    assert w["assoc"].tolist() == [-1] and w["first_hit"].tolist() == [[0]] and w["iou"].tolist() == [[0.5]]
    w = _check(cuda, _px8((0, 0, 0, 2, 2, 1)), one, s8, 10, float(np.nextafter(0.5, 0.0)), [0.5], "just under")
    assert w["assoc"].tolist() == [0]
    big = np.array([(0, 0, 0, 4, 4, 4)], np.float32)
    w = _check(cuda, _px8((0, 0, 0, 4, 4, 4)), np.repeat(big, 2, 0), s8, 10, 0.5, [0.5], "identical GT")
    assert w["assoc"].tolist() == [0, -1]
    w = _check(cuda, _px8((0, 0, 0, 4, 4, 3), (0, 0, 0, 4, 4, 4)), big, s8, 10, 0.5, [0.5, 0.8], "later better")
    assert w["assoc"].tolist() == [0] and w["first_hit"].tolist() == [[0], [1]]
    w = _check(cuda, np.zeros((2, 6), np.float32), np.array([(0, 0, 0, 1, 1, 1)], np.float32), s8, 10, 0.5, [0.5],
               "zero-padded")
    assert w["assoc"].tolist() == [0] and w["matched"].tolist() == [[0, 0, 0, 1, 1, 1]]
    rois = _px8((0, 0, 0, 2, 2, 1), (1, 1, 1, 3, 3, 3))
    a = _check(cuda, rois, np.array([(2, 2, 2, 0, 0, 0)], np.float32), s8, 10, 0.5, [0.5], "swapped GT")
    assert a["iou"].tobytes() == E.score(rois, one, s8, 10, 0.5, [0.5])["iou"].tobytes()
    w = _check(cuda, _px8((4, 0, 0, 2, 8, 8), (0, 0, 0, 4, 4, 4)), big, s8, 10, 0.5, [0.5], "invalid first row")
    assert w["counts"].tolist() == [1, 1]


def test_no_rows_padded_rows_and_nan_rows(cuda):
    _, gt = _case(1, 4, 5)
    w = _check(cuda, np.zeros((0, 6), np.float32), gt, what="R = 0")
    assert w["counts"].tolist() == [0, E.NONE] and (w["assoc"] == -1).all() and (w["first_hit"] == E.NONE).all()
    w = _check(cuda, np.zeros((300, 6), np.float32), gt, what="all padded")
    assert w["counts"].tolist() == [300, 0] and (w["assoc"] == -1).all()       # matched == 0: the no-match branch
    rois, gt = _case(2, 300, 5)
    rois[0] = np.nan
    rois[7, 4] = np.nan
    rois[CHUNK] = np.nan
    w = _check(cuda, rois, gt, what="NaN rows")
    assert w["counts"][1] == 1 and not w["iou"][:, [0, 7, CHUNK]].any()
    rois[:] = np.nan
    w = _check(cuda, rois, gt, what="all NaN")
    assert w["counts"].tolist() == [0, E.NONE]


@pytest.mark.parametrize("R", [1, 63, 65, CHUNK - 1, CHUNK, CHUNK + 1, 1025, 8000])
def test_row_counts_across_every_boundary(cuda, R):
    rois, gt = _case(10 + R, R, 50)
    w = _check(cuda, rois, gt, topk=512, what=f"R = {R}")
    n = int((w["assoc"] >= 0).sum())
    if R in (63, 1025):
        assert 0 < n < 50, n                        # some GT boxes matched, some not: the aggregation's matched branch
    if R == 8000:
        assert n == 50 and (w["first_hit"] < E.NONE).all()


@pytest.mark.parametrize("G", [1, 512])
def test_gt_count_limits(cuda, G):
    rois, gt = _case(20 + G, 700, G)
    w = _check(cuda, rois, gt, what=f"G = {G}")
    assert (w["assoc"] >= 0).any()


@pytest.mark.parametrize("T", [0, 8])
def test_grid_length_limits(cuda, T):
    rois, gt = _case(30 + T, 600, 20)
    grid = [0.05, 0.1, 0.2, 0.3, 0.4, 0.5, 0.7, 0.9][:T]
    w = _check(cuda, rois, gt, grid=grid, what=f"T = {T}")
    assert w["first_hit"].shape == (T, 20)
    # the IoU matrix is optional: without it the other outputs are the same
    got = _gpu(cuda, rois, gt, SHAPE, 512, 0.5, grid, want_iou=False)
    _assert_same(got, {k: w[k] for k in got}, "iou = NULL")


@pytest.mark.parametrize("topk", [0, 100, 599, 600, 601, 5000])
def test_topk_below_equal_and_above_the_row_count(cuda, topk):
    rois, gt = _case(40, 600, 30)
    w = _check(cuda, rois, gt, topk=topk, what=f"topk = {topk}")
    assert w["assoc"].max() < max(topk, 1) and w["counts"][0] <= min(topk, 600)
    if topk == 100:
        # a grid prefix above topk: the first hits come from all R rows, so K = 500 counts rows topk never saw
        from m3d.rpn_eval import summarize
        assert ((w["first_hit"] >= 100) & (w["first_hit"] < 500)).any()
        got = _gpu(cuda, rois, gt, SHAPE, topk, 0.5, GRID3)
        s_gpu, s_ref = (summarize([r], [0.0], [0.0], [gt], [50, 100, 500], GRID3) for r in (got, w))
        assert s_gpu == s_ref and s_ref["detection_at"]["0.30@500"] > s_ref["detection_at"]["0.30@100"]


def test_score_proposals_rows_of_a_buffer_two_runs_and_a_graph(cuda):
    """The host entry: records written into rows of one preallocated buffer
    (nothing outside a row's record is touched), a second run and a replay of
    one plain HIP-graph capture give the same bytes."""
    from m3d import rpn_eval
    rois, gt = _case(50, 6000, 50)
    want = E.score(rois, gt, SHAPE, 512, 0.5, GRID3)
    d_rois, d_gt = torch.from_numpy(rois).to(cuda)[None], torch.from_numpy(gt).to(cuda)
    n = rpn_eval.record_len(50, 3)
    buf = torch.full((3, n + 10), GUARD, dtype=torch.int32, device=cuda)
    rec, iou = rpn_eval.score_proposals(d_rois, d_gt, SHAPE, 512, 0.5, GRID3, out=buf[1], return_iou=True)
    assert rec.data_ptr() == buf[1].data_ptr() and rec.numel() == n
    again = rpn_eval.score_proposals(d_rois, d_gt, SHAPE, 512, 0.5, GRID3)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[0] == GUARD).all() and (host[2] == GUARD).all() and (host[1, n:] == GUARD).all()
    got = rpn_eval.unpack_record(host[1], 50, 3)
    got["iou"] = iou.cpu().numpy()
    _assert_same(got, want, "score_proposals")
    assert torch.equal(again, rec)
    graph = torch.cuda.CUDAGraph()
    replayed = torch.full((n,), GUARD, dtype=torch.int32, device=cuda)
    with torch.cuda.graph(graph):
        rpn_eval.score_proposals(d_rois, d_gt, SHAPE, 512, 0.5, GRID3, out=replayed)
    replayed.fill_(GUARD)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(replayed, rec)
    with pytest.raises(ValueError, match="GT boxes"):
        rpn_eval.score_proposals(d_rois, d_gt[:0], SHAPE, 512, 0.5, GRID3)


# ---------------------------------------------------------------------------
# RPN.evaluate on a two-image dataset in the reference's on-disk layout (built
# as tests/test_gpu_generator.py builds its own, with that file's configuration)
# ---------------------------------------------------------------------------
S, D = 64, 16
BOXES = [np.array([[4, 4, 2, 32, 36, 10], [30, 8, 5, 60, 34, 15], [12, 36, 0, 40, 62, 8]], np.float32),
         np.array([[8, 10, 1, 40, 30, 9], [34, 30, 6, 62, 60, 16]], np.float32)]


def _dataset(root):
    from m3d.dataset import ToyDataset
    from m3d.tiff import imwrite
    os.makedirs(os.path.join(root, "datasets"))
    rows = []
    for i, boxes in enumerate(BOXES):
        rng = np.random.default_rng(20 + i)
        raw = rng.integers(100, 4000, (D, S, S)).astype(np.uint16)
        for y1, x1, z1, y2, x2, z2 in boxes.astype(int):
            raw[z1:z2, y1:y2, x1:x2] += 9000
        paths = [os.path.join(root, f"vol_{i}{ext}") for ext in (".tiff", ".dat", ".pickle.bz2")]
        imwrite(paths[0], raw)
        with open(paths[1], "w") as f:
            for y1, x1, z1, y2, x2, z2 in boxes.astype(int):
                f.write(f"1 {z1} {y1} {x1} {z2} {y2} {x2}\n")
        with bz2.BZ2File(paths[2], "wb") as f:
            pickle.dump(np.zeros((D, S, S, len(boxes)), bool), f)
        rows.append(paths)
    with open(os.path.join(root, "datasets", "train.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["images", "cabs", "masks"])
        w.writerows(rows)
    ds = ToyDataset()
    ds.load_dataset(root, is_train=True)
    ds.prepare()
    return ds


def test_rpn_evaluate_equals_the_composition_by_hand(cuda, tmp_path):
    from m3d.config import synthetic_rpn_config
    from m3d.generator import RPNGenerator
    from m3d.model import RPN
    from m3d.rpn_eval import summarize
    cfg = synthetic_rpn_config(S, depth=D, RPN_POSITIVE_IOU=0.3, RPN_NEGATIVE_IOU=0.1, RPN_TRAIN_ANCHORS_PER_IMAGE=256,
                               PRE_NMS_LIMIT=2000, POST_NMS_ROIS_TRAINING=300, AUGMENT=False, RPN_AUGMENT_GT=False,
                               AUG_BRIGHTNESS_DELTA=0.0, EVAL_TOPK_RPN=100, EVAL_TOPK_GRID=[50, 100, 300],
                               EVAL_MATCH_IOU=0.05, EVAL_MATCH_IOU_GRID=[0.02, 0.10, 0.30])
    ds = _dataset(str(tmp_path))
    model = RPN(cfg, device=cuda, seed=1)
    got = model.evaluate(["TEST SUBSET"], [ds], seed=4)
    assert list(got) == ["test"]

    gen = RPNGenerator(cfg, ds, model.anchors.reshape(-1, 6), cuda, seed=4, shuffle=False)
    records, cls, box, gts = [], [], [], []
    with torch.no_grad():
        for k in range(len(gen)):
            image, targets = gen[k]
            out = model.forward(image, proposals=True)
            _, lc, lb = model.loss_total(out, targets)
            gts.append(np.asarray(gen.last["boxes"], np.float32))
            rois = out["rpn_rois"][0].cpu().numpy()
            assert rois.shape == (300, 6)
            records.append(E.score(rois, gts[-1], (S, S, D), 100, 0.05, cfg.EVAL_MATCH_IOU_GRID))
            cls.append(np.float32(lc.item()))
            box.append(np.float32(lb.item()))
    want = summarize(records, cls, box, gts, cfg.EVAL_TOPK_GRID, cfg.EVAL_MATCH_IOU_GRID)
    print("RPN.evaluate:", got["test"])
    assert len(gts) == 2 and all(np.array_equal(g, b) for g, b in zip(gts, BOXES))
    assert set(got["test"]) == set(want)
    for key in want:
        assert got["test"][key] == want[key], (key, got["test"][key], want[key])
    assert want["rpn_test_class_mean"] > 0 and len(want["detection_at"]) > 0
    # steps caps the subset; two subsets come back under their own keys
    two = model.evaluate(["TRAIN SUBSET", "TEST SUBSET"], [ds, ds], steps=1, seed=4)
    assert list(two) == ["train", "test"]
    assert two["train"]["rpn_train_class_mean"] == float(cls[0]) and two["train"]["rpn_train_class_std"] == 0.0
