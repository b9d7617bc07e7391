"""Every kernel path of csrc/topk.hip, csrc/nms3d.hip, csrc/rpn_targets.hip and
csrc/targets.hip at the smallest shapes that reach it, against tests/selref.py
(the restatements of oracle/heads_ref.py and oracle/ops_ref.py on inputs whose
IoUs, ties and thresholds are exact).  Everything is bit-exact except rpn_bbox
and the detection deltas (one logf and two float32 divisions): those keep the
existing 1e-5 / 2e-6 bars against the float32 restatement and are also held to
selref.delta_bound against a float64 evaluation.  tests/test_selref.py proves
on the CPU that every RPN case below reaches the branch it is named after.

Which case reaches which path
-----------------------------
csrc/topk.hip
* topk_hist_kernel / tk_state_kernel, all six digit passes, the 9-bit last pass
  alone deciding: test_topk_last_digit; the first pass alone (sign bit):
  test_topk_extreme_keys
* topk_gather_kernel, keys equal to the threshold (the `need` counter):
  test_topk_duplicates_contract; one block and several: every topk test
* rank_count_kernel<true>: INT64_MIN selected (u = 0, the DESC padding value)
  with k % 8 != 0: test_topk_extreme_keys[1-1], [9-9], [777-777]; one chunk /
  two chunks (gridDim.y 1 / 2, k = RS_CHUNK and RS_CHUNK + 1):
  test_topk_size_boundaries[5000-2048], [5000-2049]
* rank_scatter_kernel: the same; perm_init_kernel / bitonic_perm_kernel<true> /
  perm_scatter_kernel (k = RS_MAX + 1) against the last rank-sort size:
  test_topk_size_boundaries[40000-32768], [40000-32769]
* rank_count_kernel<false> (ascending, N <= 32768): every NMS test below 33000
* bitonic_perm_kernel<false> (ascending, N > 32768): test_nms_ascending_bitonic
* m3d_topk_keys workspace check: test_topk_workspace_too_small; run-to-run:
  test_topk_repeatable
* score_keys_kernel without / with gidx (-0.0 fold, +-inf, denormals):
  test_score_keys_order

csrc/nms3d.hip
* nms_keys_kernel (NaN, -inf, -FLT_MAX invalid; nextafter(-FLT_MAX, 0), +inf,
  -0.0 valid), nms_gather_kernel: test_nms_invalid_scores (valid / invalid
  boundary on a 64-row block: [*-128-64]; inside one: [*-130-70]);
  test_nms_all_invalid
* nms_mask_kernel: IoU == thr, thr 0 and 1, zero-volume and flipped boxes:
  test_nms_threshold_edges, test_nms_exact_half; diagonal / off-diagonal tiles,
  partial last tile: test_nms_chain
* nms_reduce_pf_kernel: max_out inside a block, on a block edge, 0, > N:
  test_nms_max_out; decisions carried through removed[] over five block edges:
  test_nms_chain[3d-327], [2d-327]; cb = 17 (G = 60, rows 60..63 in the second
  register slot): [3d-1029]; cb = 256 (G = 4, every slot used): [3d-16384]
* nms_reduce_kernel (cb = 257, the first LDS-list size): test_nms_chain[3d-16385];
  cb = 516 with max_out reached / an invalid tail: test_nms_ascending_bitonic
* iou2d and the 4-column gather: every [2d-*] id
* proposal_decode_kernel: bit equality with ops_ref at four image depths, +-3
  clips, zero-size anchors, boxes leaving [0, 1], each min-size line binding:
  test_proposal_decode_bits; out-of-range order rows and the err flag:
  test_proposal_decode_out_of_range; k > A, k = 0: test_proposal_decode_sizes
* proposal_gather_kernel rows past num_keep, num_keep = 0: test_proposal_gather
* the chained layer: test_proposal_layer_end_to_end

csrc/rpn_targets.hip (test_rpn_targets[<case>], both builders)
* rpn_iou_kernel / rpn_gt_best_kernel / rpn_label_kernel: every case; G = 256:
  [g256]; flipped corners: [flipped]; a GT without overlap (n == 0, arg-max on
  anchor 0) and a GT-best anchor below neg_iou, re-marked and not:
  [no-overlap], [no-overlap-minpos0]
* atss_chunk_topk_kernel: k = 24 and 64 (ATSS_KMAX), a list over two chunks
  with a partial last one and a chunk past the list: [pre-k24], [pre-k64];
  every chunk but the first past the list: [listcap-8192]
* atss_kernel without prefilter, nch == 1: [three-outcomes], [hand10-*];
  ATSS_TOPK > ATSS_KMAX with nch > 1: [nopre-k65], [nopre-k200]; topk >= A:
  [k-ge-A]; n < k (the `zeros` term): the second GT of every [pre-*] / [nopre-*]
* its three outcomes: enough candidates / the min_pos best of the top-k / a
  list shorter than min_pos completed by the lowest-index zero-IoU anchors:
  [three-outcomes], [hand10-cand], [hand10-topk], [hand10-zeros]; the same over
  the prefiltered set: [pre-minpos20], [listcap-8192]
* ties: k-th and (k+1)-th IoU bit-equal, the fallback choosing 4 of 8 equal
  IoUs by index, the stage-0 cut inside a run of equal iou_max: [ties]; eight
  IoUs bit-equal to thr (the one case with margin 0; rpn_match cannot tell
  `>=` from `>` in the mark, see selref._on_thr_case): [on-thr]
* sel_init_kernel / sel_hist_kernel / sel_pick_kernel / sel_apply_kernel:
  stage 0 active: [bal-total8], [bal-total64]; keep <= 0 in stage 0:
  [bal-ratio0]; in stage 1: [bal-ratio1]; both stages inactive:
  [bal-few-neg]; nearbyint half-even: [bal-half-even], [bal-half-odd]; two
  seeds: [bal-seed-a], [bal-seed-b] and test_rpn_seeds_differ
* count_kernel / counts_out_kernel: the builder's counts in every case
* pos_block_count_kernel / scan_kernel / pos_deltas_kernel, positives on both
  sides of two SCAN_CHUNK boundaries, rows in anchor order: [scan-chunk]
* host checks: G = 257: test_rpn_g257_rejected; ATSS_TOPK < 1:
  tests/test_capi.py::test_rpn_targets_rejects_atss_topk_below_one
* atomic list order must not show: test_rpn_repeatable

csrc/targets.hip (detection_targets_kernel)
* N = 1, 1000 (npow 1024, padding keys), 16384 (all of the LDS key array):
  test_detection_sizes; N = 16385 and G = 257: test_detection_rejections;
  G = 256: test_detection_g256
* zero rows between live rows in proposals and GT (gt_orig), duplicate GT rows
  (first max): test_detection_zero_rows_and_duplicates
* IoU == pos_thr, one ulp below, == neg_thr, one ulp below:
  test_detection_exact_thresholds
* int(float32(T) * ratio): test_detection_truncation
* no positives / no negatives / fewer live proposals than T:
  test_detection_empty_sets
* use_mini_mask on and off, B = 2 (seed + b), mask targets at (4, 4, 4):
  test_detection_layer_options
"""
import types

import numpy as np
import pytest
import torch

import selref as S
from oracle import ops_ref as R

pytestmark = pytest.mark.gpu

F = np.float32
FLT_MAX = S.FLT_MAX


def T(a, dev):
    return torch.from_numpy(np.array(a, order="C")).to(dev)          # a copy: cached inputs are read-only


def bits(a):
    return np.ascontiguousarray(np.asarray(a, F)).view(np.uint32)


def assert_bits(got, want, what=""):
    np.testing.assert_array_equal(bits(got), bits(want), err_msg=what)


# =========================================================================== top-k
def _keys64(n, seed):
    """n distinct int64 keys (the hash is a bijection of the high word)"""
    i = np.arange(n, dtype=np.uint64)
    hi = S.mix32(i * np.uint64(0x9E3779B9) + np.uint64(seed))
    lo = S.mix32(i + np.uint64(seed) * np.uint64(77))
    return ((hi << np.uint64(32)) | lo).view(np.int64)


def _topk(dev, keys, k):
    from m3d import ops
    vals, pos = ops.topk_keys(T(keys, dev), k, positions=True)
    return vals.cpu().numpy(), pos.cpu().numpy()


@pytest.mark.parametrize("n,k", [(1, 1), (9, 9), (777, 777)])
def test_topk_extreme_keys(cuda, n, k):
    keys = _keys64(n, n)
    keys[n // 2] = S.I64_MIN
    if n > 1:
        keys[n // 3] = S.I64_MAX
    assert k % 8 != 0 and len(set(keys.tolist())) == n
    vals, pos = _topk(cuda, keys, k)
    wv, wp = S.topk_sorted(keys, k)
    assert np.array_equal(vals, wv) and np.array_equal(pos, wp)
    assert vals[-1] == S.I64_MIN and pos[-1] == n // 2


@pytest.mark.parametrize("n,k", [(5000, 2048), (5000, 2049), (40000, 32768), (40000, 32769)])
def test_topk_size_boundaries(cuda, n, k):
    keys = _keys64(n, k)
    keys[17] = S.I64_MAX
    vals, pos = _topk(cuda, keys, k)
    wv, wp = S.topk_sorted(keys, k)
    assert np.array_equal(vals, wv) and np.array_equal(pos, wp)


def test_topk_last_digit(cuda):
    """The 512 largest of 3000 keys agree in every bit above the last 9-bit
    digit: the first five passes find one bin, the last alone places the cut."""
    n, k = 3000, 100
    keys = _keys64(n, 5) >> np.int64(8)                              # below 2^55
    top = S.shuffled(n, 9)[:512]
    keys[top] = (np.int64(0x123456789ABCDE) << np.int64(9)) | S.shuffled(512, 3).astype(np.int64)
    assert len(set(keys.tolist())) == n
    vals, pos = _topk(cuda, keys, k)
    wv, wp = S.topk_sorted(keys, k)
    assert np.all((wv >> 9) == 0x123456789ABCDE)
    assert np.array_equal(vals, wv) and np.array_equal(pos, wp)


def test_topk_duplicates_contract(cuda):
    """About 200 distinct values over 5000 keys, the k-th value repeated across
    the cut.  The contract on equal keys (ops.topk_keys): the values are the
    sorted reference's; keys[pos] == vals; positions are pairwise distinct; the
    positions of keys strictly above the threshold are exactly the reference
    set.  WHICH of the keys equal to the threshold are taken, and the order
    of positions among equal keys, follow atomic arrival and are not fixed."""
    n = 5000
    keys = ((S.hash_uniform((n,), 21) * 200).astype(np.int64) - 100) * np.int64(1 << 40)
    srt = np.sort(keys)[::-1]
    k = next(q for q in range(1000, n) if srt[q - 1] == srt[q] and srt[q - 1] != srt[q - 5])
    assert len(np.unique(keys)) >= 190 and srt[k - 1] == srt[k]
    vals, pos = _topk(cuda, keys, k)
    assert np.array_equal(vals, srt[:k])
    assert np.array_equal(keys[pos], vals)
    assert len(np.unique(pos)) == k
    thr = srt[k - 1]
    assert np.array_equal(np.sort(pos[vals > thr]), np.nonzero(keys > thr)[0])


def test_score_keys_order(cuda):
    from m3d import ops
    special = np.array([-0.0, 0.0, np.inf, -np.inf, 1e-45, -1e-45, 1e-39, -0.0, 0.0, -3.5, 2.0, -np.inf, np.inf],
                       F)
    n = 700
    score = ((S.hash_uniform((n,), 4) * 40).astype(np.int64) - 20).astype(F) / F(8)      # many ties, both signs
    at = S.shuffled(n, 6)[:special.size]
    score[at] = special
    probs = np.stack([np.zeros(n, F), score], 1)
    gi = S.shuffled(n, 8).astype(np.int64)
    for g in (None, gi):
        keys = ops.score_keys(T(probs, cuda), None if g is None else T(g, cuda)).cpu().numpy()
        assert len(np.unique(keys)) == n
        got = np.argsort(keys, kind="stable")[::-1]
        assert np.array_equal(got, S.score_order(score, g))
        assert np.array_equal(got, np.lexsort((np.arange(n) if g is None else g, -(score + F(0)))))
    assert np.array_equal(ops.topk_order(T(probs, cuda), n).cpu().numpy(), S.score_order(score))


def test_topk_workspace_too_small(cuda):
    import m3d._lib as lib
    L = lib.load()
    keys = T(_keys64(100, 1), cuda)
    out = torch.empty(10, device=cuda, dtype=torch.int64)
    nb = int(L.m3d_topk_workspace_bytes(100, 10))
    ws = torch.empty(nb // 8 + 1, device=cuda, dtype=torch.int64)
    for args in ((lib.ptr(ws), nb - 1), (None, nb)):
        rc = L.m3d_topk_keys(lib.ptr(keys), 100, 10, lib.ptr(out), None, args[0], args[1], lib.stream())
        assert rc == -1 and b"workspace too small" in L.m3d_last_error()
    assert L.m3d_topk_keys(lib.ptr(keys), 100, 10, lib.ptr(out), None, lib.ptr(ws), nb, lib.stream()) == 0
    assert np.array_equal(out.cpu().numpy(), S.topk_sorted(keys.cpu().numpy(), 10)[0])


def test_topk_repeatable(cuda):
    keys = _keys64(5000, 3)
    a, b = _topk(cuda, keys, 2049), _topk(cuda, keys, 2049)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# =========================================================================== NMS
def _nms(dev, boxes, scores, max_out, thr, mode):
    from m3d import ops
    keep, num = ops.non_max_suppression_3d_padded(T(boxes, dev), T(scores, dev), max_out, thr, mode=mode)
    n = int(num.item())
    assert 0 <= n <= max(max_out, 0)
    return keep.cpu().numpy()[:n]                                    # entries past num_keep are not asserted


MODES = ["3d", "2d"]
INVALID = [np.nan, -np.inf, -FLT_MAX]


def _invalid_case(N, nvalid, mode):
    boxes = S.hash_boxes(N, 11 + N, mode)
    scores = np.round(S.hash_uniform((N,), N) * 20 - 10).astype(F) / F(4)               # ties, both signs
    valid = np.sort(S.shuffled(N, 5)[:nvalid])
    scores[valid[:6]] = [np.inf, -0.0, 0.0, np.nextafter(F(-FLT_MAX), F(0)), -0.0, np.inf]
    inv = np.setdiff1d(np.arange(N), valid)
    scores[inv] = np.resize(np.array(INVALID, F), inv.size)
    return boxes, scores


@pytest.mark.parametrize("N,nvalid", [(128, 64), (130, 70)])
@pytest.mark.parametrize("mode", MODES)
def test_nms_invalid_scores(cuda, mode, N, nvalid):
    boxes, scores = _invalid_case(N, nvalid, mode)
    for thr, max_out in ((0.3, N), (1.0, N)):                        # thr 1: nothing suppressed, every valid row kept
        got = _nms(cuda, boxes, scores, max_out, thr, mode)
        want = S.nms(boxes, scores, max_out, thr, mode)
        assert np.array_equal(got, want)
        if thr == 1.0:
            assert len(got) == nvalid
    assert 0 < len(S.nms(boxes, scores, N, 0.3, mode)) < nvalid


@pytest.mark.parametrize("mode", MODES)
def test_nms_all_invalid(cuda, mode):
    boxes = S.hash_boxes(130, 3, mode)
    scores = np.resize(np.array(INVALID, F), 130)
    assert len(_nms(cuda, boxes, scores, 50, 0.5, mode)) == 0


@pytest.mark.parametrize("max_out", [1, 63, 64, 65, 200, 205, 0])
@pytest.mark.parametrize("mode", MODES)
def test_nms_max_out(cuda, mode, max_out):
    """199-box chain behind one isolated box (N = 200): sorted row 0 and the odd
    rows are kept, 101 in all -- 33 in block 0, 32 in block 1.  max_out 63 and
    64 stop inside block 1; 65 is reached by row 127, the last row of block 1;
    200 and 205 are never reached."""
    boxes, scores, kept = S.nms_chain(199, lead=1, mode=mode)
    got = _nms(cuda, boxes, scores, max_out, S.CHAIN_THR, mode)
    assert np.array_equal(got, kept[:max(max_out, 0)])
    assert np.array_equal(got, S.nms(boxes, scores, max_out, S.CHAIN_THR, mode))


@pytest.mark.parametrize("mode", MODES)
def test_nms_exact_half(cuda, mode):
    b = S.half_pair(mode)
    s = np.array([2, 1], F)
    assert np.array_equal(_nms(cuda, b, s, 2, 0.5, mode), [0, 1])                          # IoU == thr: kept
    assert np.array_equal(_nms(cuda, b, s, 2, float(np.nextafter(F(0.5), F(0))), mode), [0])


@pytest.mark.parametrize("mode", MODES)
def test_nms_threshold_edges(cuda, mode):
    """thr 0 (any overlap suppresses; IoU 0 does not) and thr 1 (nothing can),
    with zero-volume boxes (IoU defined as 0), flipped corners and duplicates."""
    N = 150
    boxes = S.hash_boxes(N, 31, mode)
    d = boxes.shape[1] // 2
    boxes[::7, d:] = boxes[::7, :d]                                  # zero volume
    boxes[3::7] = boxes[3::7][:, list(range(d, 2 * d)) + list(range(d))]                   # flipped corners
    boxes[5::11] = boxes[4::11][:len(boxes[5::11])]                  # exact duplicates (IoU 1)
    scores = S.hash_uniform((N,), 32).astype(F)
    for thr in (0.0, 1.0, 0.5):
        got = _nms(cuda, boxes, scores, N, thr, mode)
        assert np.array_equal(got, S.nms(boxes, scores, N, thr, mode)), thr
    assert len(S.nms(boxes, scores, N, 1.0, mode)) == N
    assert len(S.nms(boxes, scores, N, 0.0, mode)) < len(S.nms(boxes, scores, N, 0.5, mode)) < N


@pytest.mark.parametrize("mode,N", [("3d", 64 * 5 + 7), ("3d", 64 * 16 + 5), ("3d", 16384), ("3d", 16385),
                                    ("2d", 64 * 5 + 7)])
def test_nms_chain(cuda, mode, N):
    """N rows: one isolated box, then a chain whose kept rows are the odd sorted
    rows -- the last row of every 64-row block is kept and suppresses the first
    row of the next, so a wrong word of removed[] flips every later decision."""
    boxes, scores, kept = S.nms_chain(N - 1, lead=1, mode=mode)
    got = _nms(cuda, boxes, scores, N, S.CHAIN_THR, mode)
    assert len(kept) == 1 + N // 2
    assert np.array_equal(got, kept)
    if N < 2000:
        assert np.array_equal(got, S.nms(boxes, scores, N, S.CHAIN_THR, mode))


@pytest.mark.parametrize("form", ["mostly-invalid", "valid-max500"])
def test_nms_ascending_bitonic(cuda, form):
    """33000 boxes: the ascending bitonic permutation sort, cb = 516.  Once with
    a 300-box chain scattered among invalid rows (32700 equal all-ones keys,
    ordered by index, all behind the valid ones), once fully valid with max_out
    reached after 500 kept rows."""
    N = 33000
    if form == "valid-max500":
        boxes, scores, kept = S.nms_chain(N - 1, lead=1)
        got = _nms(cuda, boxes, scores, 500, S.CHAIN_THR, "3d")
        assert np.array_equal(got, kept[:500])
        return
    cb, cs, ck = S.nms_chain(299, lead=1)
    rows = np.sort(S.shuffled(N, 13)[:300])
    boxes = S.hash_boxes(N, 14)
    scores = np.resize(np.array(INVALID, F), N)
    boxes[rows], scores[rows] = cb, cs
    got = _nms(cuda, boxes, scores, N, S.CHAIN_THR, "3d")
    assert np.array_equal(got, rows[ck])
    assert np.array_equal(got, S.nms(boxes, scores, N, S.CHAIN_THR))


# =========================================================================== proposal stage
PSTD = (0.1, 0.1, 0.2, 0.2, 0.2, 0.1)


def _decode_inputs():
    A = 300
    lo = S.hash_uniform((A, 3), 41) * 0.8
    anchors = np.concatenate([lo, lo + 0.02 + S.hash_uniform((A, 3), 42) * 0.3], 1).astype(F)
    deltas = ((S.hash_uniform((A, 6), 43) - 0.5) * 8).astype(F)              # * std 0.1 / 0.2: within +-0.8
    deltas[::5] *= F(20)                                                      # beyond +-3 after the std multiply
    anchors[7::30, 3] = anchors[7::30, 0]                                     # zero height: y2 = y1 + eps binds
    anchors[8::30, 4] = anchors[8::30, 1]                                     # zero width:  x2 = x1 + eps binds
    anchors[9::30, 5] = anchors[9::30, 2]                                     # zero depth:  z2 = z1 + min_d binds
    anchors[10::30] = anchors[10::30][:, [0, 1, 2, 0, 1, 2]]                  # a point
    anchors[11::30, :3] -= F(0.5)                                             # leaves [0, 1] below
    anchors[12::30, 3:] += F(0.9)                                             # and above
    anchors[13::30] = [-0.5, -0.5, -0.5, -0.1, -0.1, -0.1]                    # wholly outside: clipped to the corner
    deltas[9::30] = 0
    probs = np.stack([np.zeros(A, F), S.hash_uniform((A,), 44).astype(F)], 1)
    return probs, deltas, anchors


@pytest.mark.parametrize("depth", [0.5, 1, 32, 20000])
def test_proposal_decode_bits(cuda, depth):
    """Bit equality with the ops_ref pieces, every column: the kernel's
    (float)exp((double)d) is ops_ref's float64 exp rounded once.  image_depth
    0.5 floors at 1; 20000 puts 1 / depth below the 1e-4 floor."""
    from m3d import ops
    probs, deltas, anchors = _decode_inputs()
    A = len(anchors)
    order = S.shuffled(A, 45).astype(np.int64)
    boxes, scores = ops.proposal_decode(T(probs, cuda), T(deltas, cuda), T(anchors, cuda), T(order, cuda), PSTD,
                                        depth)
    wb, ws = S.decode(probs, deltas, anchors, order, PSTD, depth)
    d = np.clip(deltas * np.asarray(PSTD, F), -3, 3)[order]
    assert np.any(np.abs(deltas * np.asarray(PSTD, F)) > 3)
    min_d = max(F(1) / max(F(depth), F(1)), F(1e-4))
    assert np.any(wb[:, 3] == wb[:, 0] + F(1e-6)) and np.any(wb[:, 4] == wb[:, 1] + F(1e-6))
    assert np.any(wb[:, 5] == wb[:, 2] + min_d) and (depth <= 1 or np.any(wb[:, 5] > wb[:, 2] + min_d))
    assert np.any(wb[:, :3] == 0) and np.any(wb[:, 3:] == 1)
    assert_bits(scores.cpu().numpy(), ws)
    got = boxes.cpu().numpy()
    bad = np.nonzero(np.any(bits(got) != bits(wb), 1))[0]
    assert bad.size == 0, (bad[:10], float(np.abs(got - wb).max()), d[bad[:3]])
    # the reference's own chain gives the same rows
    rb, rs, ridx = R.proposal_decode(probs, deltas, anchors, A, PSTD, depth)
    inv = np.empty(A, np.int64)
    inv[order] = np.arange(A)
    assert_bits(got[inv[ridx]], rb)


def test_proposal_decode_out_of_range(cuda):
    from m3d import ops
    probs, deltas, anchors = _decode_inputs()
    A = len(anchors)
    order = S.shuffled(A, 46).astype(np.int64)[:40].copy()
    order[[3, 17]] = [-1, A]
    args = [T(x, cuda) for x in (probs, deltas, anchors, order)]
    with pytest.raises(ValueError, match="is not in"):
        ops.proposal_decode(*args, PSTD, 32)
    boxes, scores = ops.proposal_decode(*args, PSTD, 32, check_indices=False)
    b, s = boxes.cpu().numpy(), scores.cpu().numpy()
    ok = np.setdiff1d(np.arange(40), [3, 17])
    wb, ws = S.decode(probs, deltas, anchors, order[ok], PSTD, 32)
    assert_bits(b[ok], wb)
    assert_bits(s[ok], ws)
    assert not b[[3, 17]].any() and np.all(s[[3, 17]] == -FLT_MAX)
    keep = _nms(cuda, b, s, 40, 1.0, "3d")                           # thr 1: every valid row is kept
    assert sorted(keep.tolist()) == ok.tolist()
    assert np.array_equal(keep, S.nms(b, s, 40, 1.0))


def test_proposal_decode_sizes(cuda):
    """k > A is the reference's top_k InvalidArgument; k = 0 is an empty gather:
    nothing is launched and empty outputs come back."""
    import m3d._lib as lib
    from m3d import ops
    probs, deltas, anchors = (T(x, cuda) for x in _decode_inputs())
    A = anchors.shape[0]
    with pytest.raises(ValueError, match="indices for"):
        ops.proposal_decode(probs, deltas, anchors, torch.zeros(A + 1, dtype=torch.int64, device=cuda), PSTD, 32)
    L = lib.load()
    sd = (lib.c_f * 6)(*PSTD)
    rc = L.m3d_proposal_decode(lib.ptr(probs), lib.ptr(deltas), lib.ptr(anchors), A, None, A + 1, sd, 32.0, None,
                               None, None, lib.stream())
    assert rc == -1 and b"more proposals than anchors" in L.m3d_last_error()
    b, s = ops.proposal_decode(probs, deltas, anchors, torch.zeros(0, dtype=torch.int64, device=cuda), PSTD, 32)
    assert tuple(b.shape) == (0, 6) and tuple(s.shape) == (0,)


def test_proposal_gather(cuda):
    from m3d import ops
    boxes = S.hash_boxes(50, 51)
    keep = S.shuffled(50, 52)[:20].astype(np.int32)
    for nk, P in ((7, 12), (20, 20), (0, 5), (12, 7)):
        out = ops.proposal_gather(T(boxes, cuda), T(keep, cuda), T(np.array([nk], np.int32), cuda), P)
        want = np.zeros((P, 6), F)
        m = min(nk, P)
        want[:m] = boxes[keep[:m]]
        assert_bits(out.cpu().numpy(), want)


def test_proposal_layer_end_to_end(cuda):
    from m3d import layers
    probs, deltas, anchors = _decode_inputs()
    probs[:, 1] = np.round(probs[:, 1] * 16) / 16                     # tied scores: the top-k's index order shows
    layer = layers.ProposalLayer(40, 0.5, 100, 1, PSTD, 32)
    out, cnt = layer([T(probs[None], cuda), T(deltas[None], cuda), T(anchors[None], cuda)], return_counts=True)
    want = R.proposal_layer(probs[None], deltas[None], anchors[None], 40, 0.5, 100, PSTD, 32)
    assert_bits(out.cpu().numpy(), want)
    assert 0 < int(cnt[0]) == int(np.any(want[0] != 0, 1).sum()) <= 40


# =========================================================================== RPN targets
def _cfg(c):
    return types.SimpleNamespace(RPN_TRAIN_ANCHORS_PER_IMAGE=c.total, RPN_POSITIVE_IOU=c.pos_iou,
                                 RPN_NEGATIVE_IOU=c.neg_iou, RPN_POSITIVE_RATIO=c.ratio, ATSS_TOPK=c.topk,
                                 ATSS_MIN_POS_PER_GT=c.min_pos, RPN_BBOX_STD_DEV=c.std)


def _rpn_both(dev, c):
    """(match, bbox) of build_rpn_targets and of RPNTargetBuilder, + the builder's counts"""
    from m3d.targets import RPNTargetBuilder, build_rpn_targets
    anchors = T(c.anchors, dev)
    m, b = build_rpn_targets(anchors, np.ones(len(c.gt), np.int32), np.array(c.gt), _cfg(c), seed=c.seed,
                             list_cap=c.list_cap)
    builder = RPNTargetBuilder(anchors, _cfg(c), max_gt=max(len(c.gt), 1), list_cap=c.list_cap)
    t = builder(T(c.gt, dev), seed=c.seed)
    builder.check()
    return (m.cpu().numpy(), b.cpu().numpy()), (t.match.cpu().numpy().astype(np.int32), t.bbox.cpu().numpy()), \
        builder.counts.cpu().numpy()


RATIOS = {}


@pytest.mark.parametrize("name", S.RPN_CASES)
def test_rpn_targets(cuda, name):
    """rpn_match bit-exact; rpn_bbox within the existing 1e-5 bar of heads_ref
    and within selref.delta_bound of the float64 evaluation (largest measured
    err / bound over all cases: CPU replay 0.35, MI355X 0.58 at [flipped])."""
    c = S.rpn_case(name)
    want_m, want_b = S.rpn_case_ref(name)
    (m, b), (m2, b2), counts = _rpn_both(cuda, c)
    assert np.array_equal(m, want_m), (int(np.sum(m != want_m)), int((m == 1).sum()), int((want_m == 1).sum()))
    assert np.array_equal(m2, m) and np.array_equal(bits(b2), bits(b))                   # the two builders agree
    assert counts.tolist() == [int((m == 1).sum()), int((m == -1).sum()), 0]
    np.testing.assert_allclose(b, want_b, rtol=1e-5, atol=1e-5)
    box, gt = S.rpn_delta_rows(c, want_m)
    n = len(box)
    assert not b[n:].any()
    if n:
        err = np.abs(b[:n].astype(np.float64) - S.deltas_f64(box, gt, c.std))
        bound = S.delta_bound(box, gt, c.std)
        RATIOS[name] = float((err / bound).max())
        print(f"rpn_bbox[{name}]: rows {n}, largest err/bound {RATIOS[name]:.3f} (max over cases so far "
              f"{max(RATIOS.values()):.3f})")
        assert np.all(err <= bound), (name, RATIOS[name])
    if name == "scan-chunk":
        assert n == 4                                                # rows in ascending anchor order, none lost


def test_rpn_seeds_differ(cuda):
    a = _rpn_both(cuda, S.rpn_case("bal-seed-a"))[0][0]
    b = _rpn_both(cuda, S.rpn_case("bal-seed-b"))[0][0]
    assert np.array_equal(a == 1, b == 1) and (a == -1).sum() == (b == -1).sum() > 0
    assert not np.array_equal(a == -1, b == -1)


def test_rpn_repeatable(cuda):
    """The IoU > 0 lists are filled in atomic order; labels and deltas must not show it."""
    c = S.rpn_case("pre-minpos20")
    r1, r2 = _rpn_both(cuda, c), _rpn_both(cuda, c)
    for x, y in zip(r1[0] + r1[1], r2[0] + r2[1]):
        assert np.array_equal(x.view(np.uint32) if x.dtype == F else x, y.view(np.uint32) if y.dtype == F else y)


def test_rpn_g257_rejected(cuda):
    from m3d.targets import build_rpn_targets
    a, gt = S.g257()
    c = S.rpn_case("g256")
    with pytest.raises(ValueError, match="G <= 256"):
        build_rpn_targets(T(a, cuda), np.ones(257, np.int32), gt, _cfg(c), seed=1)


# =========================================================================== detection targets
DSTD = (0.1, 0.1, 0.1, 0.2, 0.2, 0.2)
DRATIO = []


def _detect(dev, props, cls, gt, masks, T_, ratio, pos, neg, mini, seed, mask_shape=(4, 4, 4), check_masks=True):
    """Run the layer on a batch (lists of per-image arrays) and compare every
    image with heads_ref.detection_targets; returns the per-image references.
    Deltas: the existing 2e-6 bar against heads_ref, and selref.delta_bound
    against the float64 evaluation (largest measured err / bound on the MI355X:
    0.86, in test_detection_zero_rows_and_duplicates)."""
    from m3d.targets import DetectionTargetLayer
    layer = DetectionTargetLayer(None, T_, ratio, DSTD, mini, mask_shape, len(props), positive_iou_threshold=pos,
                                 negative_iou_threshold=neg)
    outs = layer([T(np.stack(x), dev) for x in (props, cls, gt, masks)], seed=seed)
    counts = layer.last_counts.cpu().numpy()
    refs = []
    for b in range(len(props)):
        rois, tgt, tcls, tdel, tmask = (o[b].cpu().numpy() for o in outs)
        ref = S.detection_targets(props[b], cls[b], gt[b], T_, ratio, pos, neg, DSTD, mini,
                                  (seed * 1000003 + b) & 0xFFFFFFFF)
        assert_bits(rois, ref[0], "rois")
        assert_bits(tgt, ref[1], "target gt boxes")
        assert np.array_equal(tcls, ref[2])
        pc = int((ref[5] >= 0).sum())
        nc = int(np.any(ref[0] != 0, 1).sum()) - pc
        assert counts[b].tolist() == [pc, nc]
        np.testing.assert_allclose(tdel, ref[3], rtol=2e-6, atol=2e-6)
        assert not tdel[pc:].any()
        if pc:
            err = np.abs(tdel[:pc].astype(np.float64) - S.deltas_f64(ref[0][:pc], ref[1][:pc], DSTD))
            bound = S.delta_bound(ref[0][:pc], ref[1][:pc], DSTD)
            DRATIO.append(float((err / bound).max()))
            print(f"detection deltas: rows {pc}, largest err/bound {DRATIO[-1]:.3f} (max so far {max(DRATIO):.3f})")
            assert np.all(err <= bound), DRATIO[-1]
        if check_masks:
            want = np.zeros_like(tmask)
            for r in range(pc):
                img = masks[b][..., ref[5][r]].astype(F)[None, ..., None]
                want[r] = np.round(R.crop_and_resize_3d(img, ref[4][r:r + 1], np.zeros(1, np.int32), mask_shape)[0, ..., 0])
            assert np.array_equal(tmask, want)
        refs.append((ref, pc, nc))
    return refs


@pytest.mark.parametrize("N", [1, 1000, 16384])
def test_detection_sizes(cuda, N):
    """N = 1: npow 1; 1000: 24 padding keys sort last; 16384: the whole LDS key array"""
    props, cls, gt, masks = S.detection_inputs(N, 5, 60 + N)
    if N == 1:
        props[0] = gt[2]                                             # the one proposal is a positive
    ((ref, pc, nc),) = _detect(cuda, [props], [cls], [gt], [masks], 64, 0.33, 0.5, 0.3, False, 4242)
    assert (pc, nc) == ((1, 0) if N == 1 else (21, 43))             # int(float32(64) * 0.33) = 21


def test_detection_rejections(cuda):
    from m3d.targets import DetectionTargetLayer
    layer = DetectionTargetLayer(None, 8, 0.5, DSTD, False, (4, 4, 4), 1)
    z = lambda *s, dt=torch.float32: torch.zeros(s, device=cuda, dtype=dt)
    with pytest.raises(ValueError, match="16384 proposals"):
        layer([z(1, 16385, 6), z(1, 2, dt=torch.int32), z(1, 2, 6), z(1, 4, 4, 4, 2, dt=torch.bool)])
    with pytest.raises(ValueError, match="256 GT"):
        layer([z(1, 10, 6), z(1, 257, dt=torch.int32), z(1, 257, 6), z(1, 4, 4, 4, 257, dt=torch.bool)])


def test_detection_g256(cuda):
    props, cls, gt, masks = S.detection_inputs(40, 256, 77)
    ((ref, pc, nc),) = _detect(cuda, [props], [cls], [gt], [masks], 32, 0.5, 0.5, 0.3, True, 5)
    assert pc > 0 and ref[5][:pc].max() > 64                         # GT indices from the upper part of the table


def test_detection_zero_rows_and_duplicates(cuda):
    """Zero rows BETWEEN live rows in proposals and GT: class ids, GT boxes and
    the mask assignment come from the ORIGINAL GT index.  GT rows 3 and 6 are
    identical: the first maximum (3) wins."""
    props, cls, gt, masks = S.detection_inputs(200, 9, 88)
    cls = np.arange(11, 20).astype(np.int32)                         # distinct: a wrong index shows in class_ids
    gt[[1, 4, 8]] = 0
    gt[6] = gt[3]
    props[5::9] = 0
    props[100:110] = gt[3] + F(0.01) * (S.hash_uniform((10, 6), 3) - 0.5).astype(F)
    ((ref, pc, nc),) = _detect(cuda, [props], [cls], [gt], [masks], 128, 0.5, 0.5, 0.3, False, 9)
    g = ref[5][:pc]
    assert pc > 20 and set(g.tolist()) <= {0, 2, 3, 5, 7} and 3 in g and len(set(g.tolist())) >= 3


def test_detection_exact_thresholds(cuda):
    p, gt, want = S.threshold_proposals()
    cls = np.array([1, 2], np.int32)
    masks = np.ones((4, 4, 4, 2), bool)
    ((ref, pc, nc),) = _detect(cuda, [p], [cls], [gt], [masks], 8, 0.5, 0.5, 0.25, False, 1, check_masks=False)
    assert (pc, nc) == (want.count("pos"), want.count("neg")) == (1, 1)
    assert_bits(ref[0][0], p[0])                                     # IoU == pos_thr: positive
    assert_bits(ref[0][1], p[3])                                     # one ulp below neg_thr: negative


def test_detection_truncation(cuda):
    """positive_count = int(float32(T) * ratio): (50, 0.58) gives 29 where the
    float64 product's floor is 28."""
    T_, ratio, f32, f64 = S.truncation_pair()
    assert (f32, f64) == (29, 28)
    props, cls, gt, masks = S.detection_inputs(600, 4, 99)
    ((ref, pc, nc),) = _detect(cuda, [props], [cls], [gt], [masks], T_, ratio, 0.3, 0.3, False, 3)
    assert pc == f32 and nc == T_ - f32


def test_detection_empty_sets(cuda):
    props, cls, gt, masks = S.detection_inputs(300, 4, 111)
    # no negatives (neg_thr 0: IoU < 0 never holds); T above the positives: zero-padded rows
    ((_, pc, nc),) = _detect(cuda, [props], [cls], [gt], [masks], 400, 1.0, 0.0, 0.0, False, 2)
    assert pc == 300 and nc == 0
    # no positives (pos_thr above every IoU)
    ((_, pc, nc),) = _detect(cuda, [props], [cls], [gt], [masks], 64, 0.5, 1.5, 1.5, False, 2)
    assert pc == 0 and nc == 64
    # fewer live proposals than T
    few = props.copy()
    few[20:] = 0
    ((_, pc, nc),) = _detect(cuda, [few], [cls], [gt], [masks], 64, 0.5, 0.5, 0.3, False, 2)
    assert 0 < pc + nc <= 20


@pytest.mark.parametrize("mini", [False, True])
def test_detection_layer_options(cuda, mini):
    a, b = S.detection_inputs(150, 5, 120), S.detection_inputs(150, 5, 121)
    refs = _detect(cuda, [a[0], b[0]], [a[1], b[1]], [a[2], b[2]], [a[3], b[3]], 48, 0.4, 0.5, 0.3, mini, 77)
    assert all(pc > 0 and nc > 0 for _, pc, nc in refs)
    assert not np.array_equal(refs[0][0][0], refs[1][0][0])
