"""CPU self-test of tests/selref.py: the builders against values derived by
hand, the ATSS fallback on a 10-anchor case, the two forms of the ATSS
statistics, the delta bound on a float32 replay, and -- for every RPN case of
tests/test_gpu_selection_paths.py -- that rpn_stages reports the branch the
case is named after, so an edit to a builder cannot move a case off its branch
unnoticed.  No GPU."""
import numpy as np
import pytest

import selref as S
from oracle import heads_ref as HR
from oracle import ops_ref as R

F = np.float32


def _bits(a):
    return np.asarray(a, F).view(np.uint32)


# --------------------------------------------------------------------------- NMS builders
@pytest.mark.parametrize("mode", ["3d", "2d"])
@pytest.mark.parametrize("n", [63, 64, 65, 130])
def test_chain_keeps_the_even_positions(n, mode):
    boxes, scores, kept = S.nms_chain(n, mode=mode)
    order = np.argsort(-scores, kind="stable")                 # chain position -> row
    assert np.array_equal(kept, order[0:n:2])
    b6 = boxes if mode == "3d" else np.stack([boxes[:, 0], boxes[:, 1], np.zeros(n, F), boxes[:, 2], boxes[:, 3],
                                              np.ones(n, F)], 1)
    for p in (0, n // 2, n - 3):                               # IoU(i, i+1) = 3/5, IoU(i, i+2) = 1/3, exactly
        assert F(R.iou3d(b6[order[p]], b6[order[p + 1]])) == F(3) / F(5)
        assert F(R.iou3d(b6[order[p]], b6[order[p + 2]])) == F(2) / F(6)
    assert F(3) / F(5) > F(S.CHAIN_THR) > F(2) / F(6)
    assert np.array_equal(S.nms(boxes, scores, n, S.CHAIN_THR, mode), kept)
    assert sorted(scores) == list(range(1, n + 1)) and not np.array_equal(order, np.arange(n))


def test_chain_lead_puts_a_kept_row_on_a_block_edge():
    boxes, scores, kept = S.nms_chain(64 * 5 + 7, lead=1)
    order = np.argsort(-scores, kind="stable")
    rank_of = np.empty_like(order)
    rank_of[order] = np.arange(order.size)
    kept_ranks = rank_of[kept]
    assert np.array_equal(kept_ranks, np.concatenate([[0], np.arange(1, order.size, 2)]))
    for edge in (63, 127, 191, 255, 319):                      # last row of blocks 0..4 kept: suppresses row edge + 1
        assert edge in kept_ranks and edge + 1 not in kept_ranks
    assert np.array_equal(S.nms(boxes, scores, order.size, S.CHAIN_THR), kept)


@pytest.mark.parametrize("mode", ["3d", "2d"])
def test_half_pair_is_exactly_one_half(mode):
    b = S.half_pair(mode)
    below = float(np.nextafter(F(0.5), F(0)))
    s = np.array([2, 1], F)
    assert np.array_equal(S.nms(b, s, 2, 0.5, mode), [0, 1])          # IoU == thr: not suppressed
    assert np.array_equal(S.nms(b, s, 2, below, mode), [0])           # one ulp lower: suppressed
    if mode == "3d":
        assert F(R.iou3d(b[0], b[1])) == F(0.5)


# --------------------------------------------------------------------------- detection builders
def test_threshold_proposals_sit_on_the_thresholds():
    p, gt, want = S.threshold_proposals()
    ov = HR.overlaps_graph(p, gt)
    m = ov.max(1)
    assert m[0] == F(0.5) and m[1] == np.nextafter(F(0.5), F(0))
    assert m[2] == F(0.25) and m[3] == np.nextafter(F(0.25), F(0))
    assert np.array_equal(ov.argmax(1), [0, 0, 1, 1])
    cls = ["pos" if v >= F(0.5) else ("neg" if v < F(0.25) else "none") for v in m]
    assert cls == want


def test_truncation_pair():
    T, r, a, b = S.truncation_pair()
    assert a == int(F(T) * F(r)) and b == int(np.floor(T * r)) and a != b
    assert (T, r, a, b) == (50, 0.58, 29, 28)


def test_topk_and_score_order_references():
    k = np.array([5, S.I64_MIN, 5, S.I64_MAX, -1, 5], np.int64)
    v, p = S.topk_sorted(k, 5)
    assert v.tolist() == [S.I64_MAX, 5, 5, 5, -1] and p.tolist() == [3, 0, 2, 5, 4]
    s = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1.0, 0.0], F)
    assert S.score_order(s).tolist() == [2, 4, 0, 1, 6, 5, 3]
    assert S.score_order(s, [6, 5, 4, 3, 2, 1, 0]).tolist() == [2, 4, 6, 1, 0, 5, 3]
    assert np.array_equal(S.mix32(np.arange(50)), [int(HR._mix32(i)) for i in range(50)])


# --------------------------------------------------------------------------- ATSS by hand
def test_atss_outcomes_by_hand():
    """GT = anchor 5 of ten overlapping cubes: IoUs (1/3, 1, 1/3) at anchors 4, 5,
    6.  topk 4: values (1, 1/3, 1/3, 0), mean 5/12, variance 76/576, thr =
    5/12 + sqrt(76/576) = 0.7799 > 1/3, so one candidate (anchor 5).
    min_pos 1: enough.  min_pos 2: the 2 best of the top-k, the tie between
    anchors 4 and 6 going to the lower index.  min_pos 4: the list (3 anchors)
    is shorter, anchor 0 (lowest index with IoU 0) completes it.  pos_iou 0.5
    leaves anchors 4 and 6 at 0 otherwise; everything without overlap is -1."""
    base = np.full(10, -1, np.int32)
    base[[4, 6]] = 0
    base[5] = 1
    want = {"hand10-cand": (base, "cand"), "hand10-topk": (base.copy(), "topk"), "hand10-zeros": (base.copy(), "zeros")}
    want["hand10-topk"][0][4] = 1
    want["hand10-zeros"][0][[0, 4, 6]] = 1
    for name, (match, outcome) in want.items():
        c, s = S.rpn_case(name), S.rpn_case_stages(name)
        assert np.array_equal(_bits(s["ov"][:, 0][[4, 5, 6]]), _bits([F(1) / F(3), 1, F(1) / F(3)]))
        assert s["n"] == [3] and s["outcome"] == [outcome] and s["ncand"] == [1]
        assert abs(float(s["thr"][0]) - (5 / 12 + (76 / 576) ** 0.5)) < 1e-7
        assert not s["stage0"] and not s["stage1"]
        assert np.array_equal(S.rpn_case_ref(name)[0], match), name


# --------------------------------------------------------------------------- every RPN case
@pytest.mark.parametrize("name", S.RPN_CASES)
def test_rpn_case_reaches_its_branch(name):
    c, s = S.rpn_case(name), S.rpn_case_stages(name)
    A, G = len(c.anchors), len(c.gt)
    # the mirror is the reference: same final labels
    assert np.array_equal(S.finish_stage1(s, c.seed), S.rpn_case_ref(name)[0])
    # ATSS statistics: the float32-accumulated form of the reference program gives the same thr, or at
    # least the same candidate set; and no IoU within 2 ulps of a threshold
    for g in range(G):
        assert s["same_cand"][g], (name, g)
        if "on_thr" in c.expect:                                     # the one case built to sit on its threshold
            assert s["margin"][g] == 0 and s["ncand"][g] == c.expect["on_thr"]
            assert _bits(s["thr"][g]) == _bits(s["thr32"][g]) == _bits(s["ov"][:, g].max())
        else:
            assert s["margin"][g] >= 2, (name, g, s["margin"][g])
    assert c.anchors.max() <= 1.0 and c.gt.max() <= 1.0          # normalised: build_rpn_targets rescales GT > 2
    kk, nch, pre = S.rpn_dispatch(A, c.topk, c.list_cap)
    if c.prefilter is not None:
        assert (pre, nch) == (c.prefilter, c.nch)
    if c.outcomes is not None:
        for g, o in enumerate(c.outcomes):
            assert o is None or s["outcome"][g] == o, (name, g, s["outcome"][g])
    e = c.expect
    for key in ("stage0", "stage1", "stage0_tie", "target_pos", "target_neg"):
        if key in e:
            assert s[key] == e[key], (name, key, s[key])
    if e.get("kth_tie"):
        assert all(s["kth_tie"])
    if e.get("big_list"):                                        # two chunks, the last partial; chunk 2 past the list
        assert 4096 < s["n"][0] < 8192 and nch == 3
    if e.get("short_list"):
        assert 0 < s["n"][1] < kk                                # the `zeros` term of the std
    if "k" in e:
        assert kk == e["k"] == A
    if "G" in e:
        assert G == e["G"]
    if "best_below_neg" in e:
        g = e["best_below_neg"]
        best = int(s["ov"][:, g].argmax())
        assert s["iou_max"][best] < F(c.neg_iou)
        assert s["match_atss"][best] == (1 if e["remarked"] else -1)
        assert s["outcome"][0] == "skip" and s["iou_max"][0] < F(c.neg_iou) and s["match_atss"][0] == -1
    if "positives_at" in e:
        pos = np.nonzero(S.rpn_case_ref(name)[0] == 1)[0]
        assert pos.tolist() == list(e["positives_at"])           # both sides of the 4096-anchor scan chunks
    if name == "ties":
        # the fallback picks 4 of 8 bit-equal IoUs by index, visibly: none of the 8 is positive otherwise
        eight = np.nonzero(s["ov"][:, 0] == s["ov"][:, 0].max())[0]
        assert len(eight) == 8 and s["iou_max"][eight[0]] < F(c.pos_iou) and s["pos0"] == 4
        assert np.array_equal(np.nonzero(s["match_atss"] == 1)[0], eight[:4])
        assert np.array_equal(np.nonzero(S.rpn_case_ref(name)[0] == 1)[0], eight[:2])      # stage 0: index again
    if name == "flipped":
        assert np.any(c.anchors[:, 0] > c.anchors[:, 3]) and np.any(c.gt[:, 1] > c.gt[:, 4])


def test_rpn_case_set_covers_the_three_outcomes_with_and_without_prefilter():
    seen = set()
    for name in S.RPN_CASES:
        c, s = S.rpn_case(name), S.rpn_case_stages(name)
        pre = S.rpn_dispatch(len(c.anchors), c.topk, c.list_cap)[2]
        seen |= {(pre, o) for o in s["outcome"]}
    for pre in (False, True):
        for o in ("cand", "topk", "zeros"):
            assert (pre, o) in seen, (pre, o)
    assert (False, "skip") in seen


def test_seeds_change_the_kept_negatives_only():
    a, b = S.rpn_case_ref("bal-seed-a")[0], S.rpn_case_ref("bal-seed-b")[0]
    assert np.array_equal(a == 1, b == 1) and (a == -1).sum() == (b == -1).sum() > 0
    assert not np.array_equal(a == -1, b == -1)


def test_g257_builder():
    a, gt = S.g257()
    assert gt.shape == (257, 6) and len(np.unique(gt, axis=0)) == 257


# --------------------------------------------------------------------------- delta bound
def test_delta_bound_holds_for_a_float32_replay():
    """The kernels' float32 operations with a correctly rounded log stay under
    delta_bound on the rows of every RPN case (largest err / bound: 0.35)."""
    worst = 0.0
    for name in S.RPN_CASES:
        c = S.rpn_case(name)
        box, gt = S.rpn_delta_rows(c, S.rpn_case_ref(name)[0])
        if not len(box):
            continue
        err = np.abs(S.deltas_f32_replay(box, gt, c.std).astype(np.float64) - S.deltas_f64(box, gt, c.std))
        bound = S.delta_bound(box, gt, c.std)
        assert np.all(err <= bound), name
        worst = max(worst, float((err / bound).max()))
        # heads_ref's own float32 form agrees with the replay to the existing bar
        np.testing.assert_allclose(S.rpn_case_ref(name)[1][:len(box)], S.deltas_f32_replay(box, gt, c.std),
                                   rtol=1e-5, atol=1e-5)
    print(f"delta replay: largest err/bound = {worst:.3f}")
    assert 0.0 < worst <= 1.0
