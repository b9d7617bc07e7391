"""References and deterministic input builders for the selection kernels:
csrc/topk.hip, csrc/nms3d.hip, csrc/rpn_targets.hip and csrc/targets.hip --
test infrastructure, numpy only, no GPU.

The references themselves are the restatements the project already has
(oracle/heads_ref.py, oracle/ops_ref.py); this module wraps them, adds
``rpn_stages`` (what a test needs to prove that an input reaches the branch it
is named after) and builds inputs whose interesting quantities are exact:

* every coordinate is an integer multiple of a power of two, small enough that
  differences, products of three extents, and volume sums are exact in
  float32.  An IoU is then one correctly rounded division of two exact
  numbers, so mirror-image anchors of a centred GT have bit-equal IoUs, and
  IoUs of exactly 1.0, 0.5 and 0.25 can be constructed (``half_pair``,
  ``threshold_proposals``);
* ``threshold_proposals`` also reaches the float32 just BELOW 0.5 and 0.25:
  a 4095 x 4097 x 1 box inside a 4096 x 8192 x 1 GT has the exact volume
  2^24 - 1; the float32 union (2^25 + 2^24 - 1) - (2^24 - 1) rounds twice, to
  2^25 exactly, and (2^24 - 1) / 2^25 is nextafter(0.5, 0);
* ``nms_chain`` is a 1-D chain with IoU(i, i+1) = 3/5 > thr = 1/2 > 1/3 =
  IoU(i, i+2): greedy NMS keeps exactly the even chain positions, and every
  decision depends on the one before it.  ``lead`` isolated boxes with the
  top scores shift the chain's parity against the 64-row blocks, so a KEPT
  row sits on a block's last row and its suppression crosses the block edge.

The bound on box-refinement deltas (``delta_bound``)
----------------------------------------------------
rpn_bbox and the detection deltas are box_refinement (core/utils.py:616-650)
divided by a std, in float32.  They are compared with ``deltas_f64``, the same
formula in float64 on the same float32 inputs.  With u = 2^-24 and every
float32 operation fl(x op y) = (x op y)(1 + e), |e| <= u:

centre columns, d = ((gc - c) / max(h, eps)) / std
  h  = fl(b3 - b0)                  relative error u
  c  = fl(b0 + 0.5 h)               absolute error <= 0.5 |h| u + |c| u
  gc likewise                       absolute error <= 0.5 |gh| u + |gc| u
  num = fl(gc - c)                  absolute error En <= (0.5|h| + |c| + 0.5|gh| + |gc|) u + |num| u
  den = max(h, eps)                 relative error u (eps is exact)
  one division, one division by std relative error u each
  => |err| <= (En / den + 3 u |num| / den) / std

size columns, d = log(max(gh, eps) / max(h, eps)) / std
  the argument carries 3 roundings (two differences, one division): the
  logarithm moves by at most 3u (first order); logf itself adds LOGF_ULP
  units in the last place of the result; the division by std adds u |d|
  => |err| <= (3 u + LOGF_ULP * ulp32(|log r|)) / std + u |d|

Second-order terms are covered by a factor (1 + 2^-20).  LOGF_ULP = 1 is an
ASSUMPTION: the HIP math API documents logf with a maximum error of 1 ulp; no
ROCm math documentation is installed next to this repository to confirm it.
"""
import functools
import types

import numpy as np

from oracle import heads_ref as HR
from oracle import ops_ref as R

F = np.float32
U = 2.0 ** -24
LOGF_ULP = 1.0
FLT_MAX = np.finfo(F).max
I64_MIN = np.iinfo(np.int64).min
I64_MAX = np.iinfo(np.int64).max
STD = (0.1, 0.1, 0.1, 0.2, 0.2, 0.2)


# --------------------------------------------------------------------------- thin wrappers
def rpn_targets(c):
    """heads_ref.build_rpn_targets of a case (see rpn_case)."""
    return HR.build_rpn_targets(c.anchors, c.gt, c.pos_iou, c.neg_iou, c.total, c.ratio, c.topk, c.min_pos,
                                c.std, c.seed)


def detection_targets(props, cls, gt, T, ratio, pos_thr, neg_thr, std, mini, seed):
    return HR.detection_targets(props, cls, gt, T, ratio, pos_thr, neg_thr, std, mini, seed)


def nms(boxes, scores, max_out, thr, mode="3d"):
    return R.non_max_suppression_3d(boxes, scores, max_out, thr, mode=mode)


def decode(probs, deltas, anchors, order, std, image_depth):
    """proposal_decode_kernel's rows for in-range `order` from the ops_ref pieces
    (core/models.py:391-447): boxes [k,6], scores [k]."""
    order = np.asarray(order)
    d = np.clip(deltas.astype(F) * np.asarray(std, F).reshape(1, 6), F(-3.0), F(3.0))[order]
    boxes = R.clip_boxes(R.apply_box_deltas(anchors[order].astype(F), d), [0, 0, 0, 1, 1, 1])
    eps = F(1e-6)
    min_d = max(F(1.0) / max(F(image_depth), F(1.0)), F(1e-4))
    boxes[:, 3] = np.maximum(boxes[:, 3], boxes[:, 0] + eps)
    boxes[:, 4] = np.maximum(boxes[:, 4], boxes[:, 1] + eps)
    boxes[:, 5] = np.maximum(boxes[:, 5], boxes[:, 2] + F(min_d))
    return boxes.astype(F), probs[order, 1].astype(F)


def topk_sorted(keys, k):
    """(values, positions) of the k largest int64 keys, descending, equal keys
    by lower position (numpy stable sort; no float conversion)."""
    keys = np.ascontiguousarray(keys, np.int64)
    u = keys.view(np.uint64) ^ np.uint64(1 << 63)            # unsigned order == signed order
    order = np.argsort(~u, kind="stable")[:k]                # descending, lower position first
    return keys[order], order


def score_order(score, global_index=None):
    """Order of m3d_score_keys[_mapped] keys, descending: score desc (-0.0 == +0.0),
    then lower (global) index."""
    s = np.asarray(score, F) + F(0.0)                        # -0.0 + 0.0 = +0.0
    gi = np.arange(s.size) if global_index is None else np.asarray(global_index)
    return np.lexsort((gi, -s.astype(np.float64)))


# --------------------------------------------------------------------------- hashes
_M32 = np.uint64(0xFFFFFFFF)


def mix32(x):
    """Vectorised lowbias32 finaliser (heads_ref._mix32)."""
    x = np.asarray(x, np.uint64) & _M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & _M32
    x = x ^ (x >> np.uint64(16))
    return x


def shuffled(n, seed):
    """A fixed permutation of range(n)."""
    return np.argsort(mix32(np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B9) + np.uint64(seed)),
                      kind="stable")


def hash_uniform(shape, seed):
    """float64 in [0, 1) from the hash of (seed, element index): fixed inputs
    that depend on no random generator's version"""
    n = int(np.prod(shape))
    h = mix32(np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B9) + np.uint64(seed) * np.uint64(0x85EBCA6B))
    return (h.astype(np.float64) / 2.0 ** 32).reshape(shape)


def hash_boxes(n, seed, mode="3d", lo=0.7, smin=0.05, smax=0.35):
    """[n, 6] (or [n, 4] in 2-D mode) float32 boxes with moderate overlaps"""
    d = 3 if mode == "3d" else 2
    a = hash_uniform((n, d), seed) * lo
    return np.concatenate([a, a + smin + hash_uniform((n, d), seed + 1) * (smax - smin)], 1).astype(F)


def detection_inputs(N, G, seed, H=8, W=8, D=4):
    """(proposals [N,6], class ids [G], gt [G,6], masks [H,W,D,G]): two thirds of
    the proposals are jittered copies of a GT, the rest wide boxes."""
    glo = 0.05 + hash_uniform((G, 3), seed) * 0.55
    gt = np.concatenate([glo, glo + 0.15 + hash_uniform((G, 3), seed + 1) * 0.2], 1)
    pick = (hash_uniform((N,), seed + 2) * G).astype(np.int64)
    jit = (hash_uniform((N, 6), seed + 3) - 0.5) * np.where(np.arange(N) % 3 == 0, 1.0, 0.12)[:, None]
    b = np.clip(gt[pick] + jit, 0, 1)
    props = np.concatenate([np.minimum(b[:, :3], b[:, 3:]), np.maximum(b[:, :3], b[:, 3:]) + 0.01], 1)
    cls = (1 + (hash_uniform((G,), seed + 4) * 3).astype(np.int32)).astype(np.int32)
    masks = hash_uniform((H, W, D, G), seed + 5) > 0.5
    return np.clip(props, 0, 1).astype(F), cls, gt.astype(F), masks


# --------------------------------------------------------------------------- anchors
UNIT = 2.0 ** -8


def varied_grid(A, dims, step=3, smin=4, smod=29, unit=UNIT):
    """[A,6] float32 anchors: lower corners on a regular grid (step units), extents
    smin + hash % smod units per axis -- few equal IoUs.  Row-major over dims."""
    n = int(np.prod(dims))
    assert A <= n
    idx = np.arange(A)
    lo = np.stack(np.unravel_index(idx, dims), 1) * step
    size = smin + (mix32(idx[:, None] * 3 + np.arange(3)[None] + 12345) % np.uint64(smod)).astype(np.int64)
    out = np.concatenate([lo, lo + size], 1) * unit
    assert out.max() <= 1.0
    return out.astype(F)


def uniform_grid(dims, size, step, unit=2.0 ** -6):
    """Equal cubes of `size` units on a regular grid: mirror images tie bit for bit."""
    idx = np.arange(int(np.prod(dims)))
    lo = np.stack(np.unravel_index(idx, dims), 1) * step
    out = np.concatenate([lo, lo + size], 1) * unit
    assert out.max() <= 1.0
    return out.astype(F)


def ubox(*v, unit=UNIT):
    return (np.asarray(v, np.float64) * unit).astype(F)


# --------------------------------------------------------------------------- rpn_stages
def _ulps(a, b):
    """distance in float32 units in the last place between non-negative floats"""
    return np.abs(np.asarray(a, F).view(np.int32).astype(np.int64) - np.asarray(b, F).view(np.int32).astype(np.int64))


def rpn_dispatch(A, topk, list_cap=None):
    """(k, nch, prefilter) as rpn_targets_impl computes them."""
    cap = int(list_cap or A)
    kk = min(topk, A)
    nch = (cap + 4095) // 4096
    return kk, nch, (1 <= kk <= 64 and nch > 1)


def rpn_stages(anchors, gt, pos_iou, neg_iou, total, ratio, topk, min_pos):
    """Mirror of heads_ref.build_rpn_targets that reports the branch data.

    Per GT (lists of length G): n (anchors with IoU > 0), k, thr (float32, the
    float64-sum form of heads_ref and the kernel), thr32 (np.mean / np.std of
    the float32 vector, the reference program's form), ncand, ncand32,
    same_cand, fallback, outcome ('skip' | 'cand' | 'topk' | 'zeros'),
    kth_tie (k-th and (k+1)-th IoU bit-equal and > 0), margin (ulps between
    thr and the nearest IoU of the column; inf for a skipped GT).
    Balancing: pos0 / neg0 (before stage 0), target_pos, stage0 (active),
    stage0_tie (equal iou_max across the cut), pos1 / neg1 (before stage 1),
    target_neg, stage1 (active).  Also ov, iou_max, match_atss (labels before
    balancing) and match_before_stage1; finish_stage1 gives the final labels,
    which test_selref.py holds equal to heads_ref's."""
    f = F
    anchors = np.asarray(anchors, f)
    gt = np.asarray(gt, f).reshape(-1, 6)
    A, G = len(anchors), len(gt)
    ov = HR.compute_overlaps_3d(anchors, gt)
    iou_max = ov.max(1)
    match = np.zeros(A, np.int32)
    match[ov.argmax(0)] = 1
    match[iou_max < f(neg_iou)] = -1
    match[iou_max >= f(pos_iou)] = 1
    s = dict(n=[], k=[], thr=[], thr32=[], ncand=[], ncand32=[], same_cand=[], fallback=[], outcome=[],
             kth_tie=[], margin=[], ov=ov, iou_max=iou_max)
    k = min(topk, A)
    for g in range(G):
        ious = ov[:, g]
        n = int(np.sum(ious > 0))
        s["n"].append(n)
        s["k"].append(k)
        if n == 0:
            for key, v in (("thr", None), ("thr32", None), ("ncand", 0), ("ncand32", 0), ("same_cand", True),
                           ("fallback", False), ("outcome", "skip"), ("kth_tie", False), ("margin", np.inf)):
                s[key].append(v)
            continue
        full = np.lexsort((np.arange(A), -ious))
        order = full[:k]
        v32 = ious[order]
        v64 = v32.astype(np.float64)
        thr = f(max(pos_iou, float(f(v64.mean())) + float(f(v64.std()))))
        thr32 = f(max(pos_iou, float(np.mean(v32)) + float(np.std(v32))))
        cand = np.nonzero(ious >= thr)[0]
        cand32 = np.nonzero(ious >= thr32)[0]
        fb = cand.size < min_pos
        if fb:
            cand = order[:min_pos]
        if cand32.size < min_pos:
            cand32 = order[:min_pos]
        match[cand] = 1
        s["thr"].append(thr)
        s["thr32"].append(thr32)
        s["ncand"].append(int(np.sum(ious >= thr)))
        s["ncand32"].append(int(np.sum(ious >= thr32)))
        s["same_cand"].append(bool(np.array_equal(np.sort(cand), np.sort(cand32))))
        s["fallback"].append(bool(fb))
        s["outcome"].append("cand" if not fb else ("topk" if n >= min(min_pos, k) else "zeros"))
        s["kth_tie"].append(bool(k < A and ious[full[k]] > 0 and
                                 ious[full[k - 1]].view(np.uint32) == ious[full[k]].view(np.uint32)))
        s["margin"].append(int(_ulps(ious, thr).min()))
    s["match_atss"] = match.copy()
    target_pos = int(round(total * ratio))
    pos = np.nonzero(match == 1)[0]
    s.update(pos0=int(pos.size), neg0=int(np.sum(match == -1)), target_pos=target_pos,
             stage0=bool(pos.size > target_pos), stage0_tie=False)
    if pos.size > target_pos:
        srt = pos[np.lexsort((pos, -iou_max[pos]))]
        if 0 < target_pos:
            s["stage0_tie"] = bool(iou_max[srt[target_pos - 1]].view(np.uint32) ==
                                   iou_max[srt[target_pos]].view(np.uint32))
        match[srt[target_pos:]] = 0
    neg = np.nonzero(match == -1)[0]
    npos = int(np.sum(match == 1))
    target_neg = int(min(len(neg), total - npos))
    s.update(pos1=npos, neg1=int(len(neg)), target_neg=target_neg, stage1=bool(len(neg) > target_neg))
    s["match_before_stage1"] = match.copy()
    return s


def finish_stage1(s, seed):
    """The final labels from rpn_stages' state: keep the target_neg negatives
    with the smallest (hash, -index) keys (heads_ref.neg_keys)."""
    match = s["match_before_stage1"].copy()
    neg = np.nonzero(match == -1)[0]
    if len(neg) > s["target_neg"]:
        h = mix32((neg.astype(np.uint64) * np.uint64(0x9E3779B9)) ^ np.uint64(seed)).astype(np.int64)
        srt = neg[np.lexsort((-neg, h))]
        match[srt[max(s["target_neg"], 0):]] = 0
    return match


# --------------------------------------------------------------------------- deltas
def deltas_f64(box, gt, std):
    """box_refinement / std in float64 on float32 inputs."""
    b = np.asarray(box, F).astype(np.float64)
    g = np.asarray(gt, F).astype(np.float64)
    eps = float(F(1e-6))
    out = np.zeros((len(b), 6))
    for q in range(3):
        h, gh = b[:, q + 3] - b[:, q], g[:, q + 3] - g[:, q]
        c, gc = b[:, q] + 0.5 * h, g[:, q] + 0.5 * gh
        out[:, q] = (gc - c) / np.maximum(h, eps)
        out[:, q + 3] = np.log(np.maximum(gh, eps) / np.maximum(h, eps))
    return out / np.asarray(std, F).astype(np.float64)


def delta_bound(box, gt, std):
    """Elementwise bound on |float32 deltas - deltas_f64| (module docstring)."""
    b = np.asarray(box, F).astype(np.float64)
    g = np.asarray(gt, F).astype(np.float64)
    sd = np.asarray(std, F).astype(np.float64)
    eps = float(F(1e-6))
    out = np.zeros((len(b), 6))
    for q in range(3):
        h, gh = b[:, q + 3] - b[:, q], g[:, q + 3] - g[:, q]
        c, gc = b[:, q] + 0.5 * h, g[:, q] + 0.5 * gh
        num, den = gc - c, np.maximum(h, eps)
        en = (0.5 * np.abs(h) + np.abs(c) + 0.5 * np.abs(gh) + np.abs(gc)) * U + np.abs(num) * U
        out[:, q] = (en / den + 3 * U * np.abs(num) / den) / sd[q]
        lg = np.log(np.maximum(gh, eps) / den)
        ulp = np.spacing((np.abs(lg) + 4 * U).astype(F)).astype(np.float64)
        out[:, q + 3] = (3 * U + LOGF_ULP * ulp) / sd[q + 3] + U * np.abs(lg / sd[q + 3])
    return out * (1 + 2.0 ** -20)


def deltas_f32_replay(box, gt, std):
    """The kernels' float32 operations with a correctly rounded log (float64 log
    rounded once): the CPU replay that test_selref.py holds under delta_bound."""
    b, g, sd = np.asarray(box, F), np.asarray(gt, F), np.asarray(std, F)
    eps = F(1e-6)
    out = np.zeros((len(b), 6), F)
    for q in range(3):
        h, gh = b[:, q + 3] - b[:, q], g[:, q + 3] - g[:, q]
        c, gc = b[:, q] + F(0.5) * h, g[:, q] + F(0.5) * gh
        out[:, q] = ((gc - c) / np.maximum(h, eps)) / sd[q]
        r = np.maximum(gh, eps) / np.maximum(h, eps)
        out[:, q + 3] = np.log(r.astype(np.float64)).astype(F) / sd[q + 3]
    return out


def rpn_delta_rows(c, match):
    """(anchor rows, GT rows) behind the rpn_bbox rows of final labels `match`."""
    pos = np.nonzero(match == 1)[0][:c.total]
    ov = HR.compute_overlaps_3d(c.anchors, c.gt)
    return c.anchors[pos], c.gt[ov[pos].argmax(1)]


# --------------------------------------------------------------------------- RPN cases
def _case(anchors, gt, pos_iou=0.3, neg_iou=0.05, total=64, ratio=0.5, topk=24, min_pos=4, seed=7,
          list_cap=None, outcomes=None, prefilter=None, nch=None, **expect):
    return types.SimpleNamespace(anchors=anchors, gt=np.asarray(gt, F).reshape(-1, 6), pos_iou=pos_iou,
                                 neg_iou=neg_iou, total=total, ratio=ratio, topk=topk, min_pos=min_pos, seed=seed,
                                 list_cap=list_cap, std=STD, outcomes=outcomes, prefilter=prefilter, nch=nch,
                                 expect=expect)


@functools.lru_cache(maxsize=None)
def _a1000():
    return varied_grid(1000, (10, 10, 10))


@functools.lru_cache(maxsize=None)
def _a9000():
    return varied_grid(9000, (30, 30, 10))


def _near(anchor, grow=1):
    """a GT that fits `anchor` well: its box with the upper corner moved by `grow` units"""
    g = np.asarray(anchor, np.float64).copy()
    g[3:] += grow * UNIT
    return g.astype(F)


GT_HUGE = (0, 0, 0, 60, 60, 60)        # best IoU <= 32^3 / 60^3 = 0.15: no candidate at pos_iou 0.3
GT_TINY1 = (0, 0, 0, 1, 1, 1)          # overlaps anchor 0 only (anchor 1 starts at 3 units)
GT_TINY8 = (0, 0, 0, 4, 4, 4)          # overlaps the 2 x 2 x 2 anchors at 0 and 3 units
GT_BIG = (0, 0, 0, 66, 66, 60)         # 22 x 22 x 10 = 4840 anchors of the 30 x 30 x 10 grid


def _three():
    a = _a1000()
    return a, np.stack([_near(a[555]), ubox(*GT_HUGE), ubox(*GT_TINY1)])


def _pre():
    a = _a9000()
    gt = np.stack([ubox(*GT_BIG), ubox(*GT_TINY8), _near(a[4444])])
    return a, gt


def _grid_gts(a, G, stride):
    """G distinct small GTs, each a shrunk copy of anchor stride * i + 7"""
    rows = a[np.arange(G) * stride + 7].astype(np.float64)
    rows[:, 3:] -= UNIT
    return rows.astype(F)


def _tie_case():
    """Centred GT on a uniform grid: its 8 mirror-image anchors hold the top 8
    IoUs, bit-equal and below pos_iou.  topk is the first k >= 8 whose k-th and
    (k+1)-th IoU are bit-equal.  No anchor reaches thr, so the fallback marks
    the 4 lowest-index anchors of the 8 -- the only positives, all with the
    same iou_max -- and stage 0 (target_pos 2) cuts inside that run."""
    a = uniform_grid((8, 8, 8), 4, 2)                                  # extents 0 .. 18 units of 2^-6
    gt = (np.array([[6, 6, 6, 12, 12, 12]]) * 2.0 ** -6).astype(F)     # centre 9 = the grid's centre
    iou = HR.compute_overlaps_3d(a, gt)[:, 0]
    srt = np.sort(iou)[::-1]
    assert srt[0] == srt[7] > srt[8] and srt[0] < F(0.4)
    topk = next(k for k in range(8, 200) if srt[k - 1] == srt[k] and srt[k] > 0)
    return _case(a, gt, pos_iou=0.4, neg_iou=0.02, total=4, ratio=0.5, topk=topk, min_pos=4,
                 outcomes=["topk"], kth_tie=True, stage0=True, stage0_tie=True, target_pos=2)


def _on_thr_case():
    """The one case built to sit ON the ATSS threshold: the 8 mirror-image anchors
    of the centred GT hold the top 8 IoUs, bit-equal, so with topk 8 the mean is
    that value and the std 0 in any arithmetic (8 v / 8 = v exactly) and thr == v:
    `IoU >= thr` counts eight candidates.  The labels cannot tell `>=` from `>`
    here or anywhere: thr >= pos_iou, so an anchor at or above thr is positive
    already, and a fallback caused by `>` would only re-mark such anchors."""
    t = _tie_case()
    return _case(t.anchors, t.gt, pos_iou=0.1, neg_iou=0.02, total=64, topk=8, min_pos=4, outcomes=["cand"],
                 on_thr=8)


def _scan_case():
    a = varied_grid(8200, (41, 20, 10))
    gt = np.stack([_near(a[i]) for i in (4095, 4096, 8191, 8192)])
    return _case(a, gt, pos_iou=0.7, neg_iou=0.05, total=256, ratio=0.5, topk=9, min_pos=1,
                 positives_at=(4095, 4096, 8191, 8192))


def _flip_case():
    a = _a1000().copy()
    sw = np.arange(0, 1000, 3)
    a[sw] = a[sw][:, [3, 4, 5, 0, 1, 2]]                               # every third anchor: corners swapped
    a[1::3, 0], a[1::3, 3] = a[1::3, 3].copy(), a[1::3, 0].copy()      # and a y-only swap
    gt = np.stack([_near(_a1000()[555])[[3, 4, 5, 0, 1, 2]], _near(_a1000()[222])[[0, 4, 2, 3, 1, 5]],
                   _near(_a1000()[777])])
    return _case(a, gt)


def _hand10(min_pos):
    """Ten 4 x 4 x 4 anchors at z = 0, 2, 4, ... (units of 2^-6) and GT = anchor 5:
    IoU 1 with anchor 5, exactly 1/3 with anchors 4 and 6, 0 elsewhere."""
    a = (np.array([[0, 0, 2 * i, 4, 4, 2 * i + 4] for i in range(10)]) * 2.0 ** -6).astype(F)
    return _case(a, a[5:6].copy(), pos_iou=0.5, neg_iou=0.05, total=100, topk=4, min_pos=min_pos,
                 prefilter=False, nch=1)


_RPN = {
    "hand10-cand": lambda: _hand10(1),
    "hand10-topk": lambda: _hand10(2),
    "hand10-zeros": lambda: _hand10(4),
    # no prefilter, nch == 1: one GT per ATSS outcome
    "three-outcomes": lambda: _case(*_three(), outcomes=["cand", "topk", "zeros"], prefilter=False, nch=1),
    # explicit list_cap 8192 at A = 1000: prefilter with chunk 1 entirely past every list
    "listcap-8192": lambda: _case(*_three(), list_cap=8192, outcomes=["cand", "topk", "zeros"], prefilter=True,
                                  nch=2),
    # prefilter: a list over two chunks (partial last) and a GT with n < k
    "pre-k24": lambda: _case(*_pre(), topk=24, prefilter=True, nch=3, big_list=True, short_list=True),
    "pre-k64": lambda: _case(*_pre(), topk=64, prefilter=True, nch=3, big_list=True, short_list=True),
    "nopre-k65": lambda: _case(*_pre(), topk=65, prefilter=False, nch=3, big_list=True, short_list=True),
    "nopre-k200": lambda: _case(*_pre(), topk=200, prefilter=False, nch=3, big_list=True, short_list=True),
    "pre-minpos20": lambda: _case(*_pre(), topk=24, min_pos=20, prefilter=True, nch=3,
                                  outcomes=["topk", "zeros", None]),
    # topk >= A
    "k-ge-A": lambda: _case(varied_grid(50, (5, 5, 2)), np.stack([_near(varied_grid(50, (5, 5, 2))[20]),
                                                                   ubox(*GT_TINY1)]),
                            topk=64, prefilter=False, nch=1, k=50),
    # n == 0 (zero-volume GT: arg-max lands on anchor 0, which neg_iou then overrides) and a GT whose best
    # anchor is below neg_iou, re-marked by the ATSS fallback ...
    "no-overlap": lambda: _case(_a1000(), np.stack([ubox(40, 40, 40, 40, 40, 40), ubox(*GT_HUGE),
                                                    _near(_a1000()[555])]),
                                neg_iou=0.2, outcomes=["skip", "topk", "cand"], best_below_neg=1, remarked=True),
    # ... and not re-marked (min_pos 0: no fallback), so the override to -1 stands
    "no-overlap-minpos0": lambda: _case(_a1000(), np.stack([ubox(40, 40, 40, 40, 40, 40), ubox(*GT_HUGE),
                                                            _near(_a1000()[555])]),
                                        neg_iou=0.2, min_pos=0, outcomes=["skip", "cand", "cand"],
                                        best_below_neg=1, remarked=False),
    "ties": _tie_case,
    "on-thr": _on_thr_case,
    # balancing on many positives (pos_iou 0.1)
    "bal-total8": lambda: _case(*_three(), pos_iou=0.1, total=8, stage0=True, stage1=True),
    "bal-total64": lambda: _case(*_three(), pos_iou=0.1, total=64, stage0=True, stage1=True),
    "bal-ratio0": lambda: _case(*_three(), pos_iou=0.1, total=64, ratio=0.0, stage0=True, target_pos=0),
    "bal-ratio1": lambda: _case(*_three(), pos_iou=0.1, total=8, ratio=1.0, stage0=True, target_neg=0,
                                stage1=True),
    "bal-few-neg": lambda: _case(*_three(), total=2000, stage0=False, stage1=False),
    "bal-seed-a": lambda: _case(*_three(), seed=1, stage1=True),
    "bal-seed-b": lambda: _case(*_three(), seed=2, stage1=True),
    "bal-half-even": lambda: _case(*_three(), pos_iou=0.1, total=5, target_pos=2, stage0=True),   # round(2.5)
    "bal-half-odd": lambda: _case(*_three(), pos_iou=0.1, total=7, target_pos=4, stage0=True),    # round(3.5)
    "scan-chunk": _scan_case,
    "g256": lambda: _case(varied_grid(10000, (25, 20, 20)), _grid_gts(varied_grid(10000, (25, 20, 20)), 256, 39),
                          total=512, G=256),
    "flipped": _flip_case,
}
RPN_CASES = list(_RPN)


@functools.lru_cache(maxsize=None)
def rpn_case(name):
    c = _RPN[name]()
    c.name = name
    for a in (c.anchors, c.gt):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def rpn_case_stages(name):
    c = rpn_case(name)
    return rpn_stages(c.anchors, c.gt, c.pos_iou, c.neg_iou, c.total, c.ratio, c.topk, c.min_pos)


@functools.lru_cache(maxsize=None)
def rpn_case_ref(name):
    m, b = rpn_targets(rpn_case(name))
    m.setflags(write=False)
    b.setflags(write=False)
    return m, b


def g257():
    a = varied_grid(10000, (25, 20, 20))
    return a, _grid_gts(a, 257, 38)


# --------------------------------------------------------------------------- NMS builders
CHAIN_THR = 0.5


def nms_chain(n, lead=0, mode="3d", seed=1):
    """(boxes, scores, kept): a chain of n boxes of width 4 at unit steps (IoU 3/5
    with the neighbour, 1/3 with the one after) behind `lead` isolated boxes;
    scores descend along (leads, chain); rows sit in a shuffled index order.
    kept = the indices greedy NMS at CHAIN_THR keeps, in selection order:
    every lead, then the even chain positions."""
    tot = n + lead
    x = np.concatenate([-100.0 - 10.0 * np.arange(lead), np.arange(n, dtype=np.float64)])
    if mode == "3d":
        b = np.stack([x, np.zeros(tot), np.zeros(tot), x + 4, np.ones(tot), np.ones(tot)], 1)
    else:
        b = np.stack([x, np.zeros(tot), x + 4, np.ones(tot)], 1)
    perm = shuffled(tot, seed)
    boxes = np.zeros_like(b, dtype=F)
    scores = np.zeros(tot, F)
    boxes[perm] = b.astype(F)
    scores[perm] = (tot - np.arange(tot)).astype(F)
    kept_rank = np.concatenate([np.arange(lead), lead + np.arange(0, n, 2)])
    return boxes, scores, perm[kept_rank].astype(np.int32)


def half_pair(mode="3d"):
    """two boxes with IoU exactly 0.5 (unit cube inside a 2 x 1 x 1 box)"""
    if mode == "3d":
        return np.array([[0, 0, 0, 1, 1, 1], [0, 0, 0, 2, 1, 1]], F)
    return np.array([[0, 0, 1, 1], [0, 0, 2, 1]], F)


# --------------------------------------------------------------------------- detection builders
def threshold_proposals():
    """(proposals [4,6], gt [2,6], expected class per proposal) at pos_thr 0.5 /
    neg_thr 0.25: IoU exactly 0.5 -> positive; nextafter(0.5, 0) -> neither;
    exactly 0.25 -> neither; nextafter(0.25, 0) -> negative (module docstring)."""
    s = 2.0 ** -14
    gt = np.array([[0, 0, 0, 4096, 8192, 1], [0, 0, 8, 4096, 16384, 9]]) * s
    p = np.array([[0, 0, 0, 4096, 4096, 1], [0, 0, 0, 4095, 4097, 1],
                  [0, 0, 8, 4096, 4096, 9], [0, 0, 8, 4095, 4097, 9]]) * s
    return p.astype(F), gt.astype(F), ["pos", "none", "none", "neg"]


def truncation_pair():
    """(T, ratio) with int(float32(T) * float32(ratio)) != floor of the float64
    product: the kernel must follow the float32 form (core/models.py casts
    TRAIN_ROIS_PER_IMAGE to float32 before the multiply)."""
    for T in range(2, 400):
        for j in range(1, 100):
            r = j / 100.0
            a, b = int(F(T) * F(r)), int(np.floor(T * r))
            if a != b:
                return T, r, a, b
    raise AssertionError("no pair found")
