"""numpy float64 restatement of detection unmolding and mask-IoU evaluation:
unmold_detections / unmold_small_3d_mask (core/models.py:7198-7419),
compute_overlaps_masks (core/utils.py:312-334) and compute_matches /
compute_ap (core/utils.py:1160-1248), in the operation order the kernels of
csrc/unmold.hip use, so the integer outputs, the thresholds and the IoU agree
bit for bit (tests/test_unmoldref.py pins this file, tests/test_gpu_unmold.py
compares the kernels with it).

Every scalar is IEEE float64 computed from the float32 inputs; every
expression below is written in the order it is evaluated.
"""
import numpy as np

OK, NOT_KEPT, RANGE, FLAT, FAINT, EMPTY, SPARSE = range(7)
STATUS_NAMES = ("OK", "NOT_KEPT", "RANGE", "FLAT", "FAINT", "EMPTY", "SPARSE")
STAT_NAMES = ("min", "max", "mean", "std", "p50", "p95", "thr", "resize_thr")


# ---- (a) box and keep filter ------------------------------------------------
def box_and_keep(det, shape):
    """det [8] float32 (normalised box, class id, score) -> (keep, box_i [6],
    class id)."""
    det = np.asarray(det, np.float32)
    H, W, D = (int(v) for v in shape)
    scale = np.array([H, W, D, H, W, D], np.float32)
    b = det[:6] * scale                                         # float32 products
    cid = int(det[6])
    ext = b[3:] - b[:3]                                         # float32 differences
    keep = cid > 0 and bool((ext > np.float32(0.5)).all())
    box = np.zeros(6, np.int32)
    if keep:
        for a, size in enumerate((H, W, D)):
            lo = int(min(max(np.floor(float(b[a])), 0.0), size - 1.0))
            hi = int(min(max(np.ceil(float(b[a + 3])), lo + 1.0), float(size)))
            box[a], box[a + 3] = lo, hi
    return keep, box, cid


# ---- (b) statistics ---------------------------------------------------------
def percentile(s, q):
    """s: sorted float64 values."""
    n = len(s)
    h = (n - 1) * (q / 100.0)
    i = int(np.floor(h))
    g = h - i
    return s[i] + (s[min(i + 1, n - 1)] - s[i]) * g


def otsu_bins(x, lo, hi):
    return np.minimum(255, np.floor(((x - lo) / (hi - lo)) * 256.0).astype(np.int64))


def otsu_threshold(x, lo, hi):
    """Unclipped Otsu threshold of float64 values x over 256 equal bins on [lo, hi]."""
    counts = np.bincount(otsu_bins(x, lo, hi), minlength=256).astype(np.float64)
    centers = lo + (np.arange(256) + 0.5) * ((hi - lo) / 256.0)
    w1 = np.cumsum(counts)
    w2 = np.cumsum(counts[::-1])[::-1]
    cc = counts * centers
    with np.errstate(divide="ignore", invalid="ignore"):
        mu1 = np.cumsum(cc) / w1
        mu2 = np.cumsum(cc[::-1])[::-1] / w2
        d = mu1[:-1] - mu2[1:]
        v = (w1[:-1] * w2[1:]) * (d * d)
    v = np.where(np.isnan(v), -np.inf, v)
    return centers[int(np.argmax(v))]


def label_min(b):
    """Face-connected components of a bool grid: every set voxel gets the
    smallest flat index of its component, unset voxels get b.size."""
    n = b.size
    lab = np.where(b, np.arange(n).reshape(b.shape), n)
    while True:
        new = lab.copy()
        for ax in range(3):
            for sh in (1, -1):
                r = np.full_like(lab, n)
                src = [slice(None)] * 3
                dst = [slice(None)] * 3
                src[ax] = slice(0, -1) if sh == 1 else slice(1, None)
                dst[ax] = slice(1, None) if sh == 1 else slice(0, -1)
                r[tuple(dst)] = lab[tuple(src)]
                new = np.minimum(new, r)
        new = np.where(b, new, n)
        if np.array_equal(new, lab):
            return lab
        lab = new


def clean_components(b):
    """(d): (cleaned grid, number of components, number removed)."""
    n = b.size
    lab = label_min(b)
    roots, sizes = np.unique(lab[b], return_counts=True)
    if len(roots) <= 1:
        return b.copy(), len(roots), 0
    min_size = max(2, int(n * 0.0002))
    small = roots[sizes < min_size]
    return b & ~np.isin(lab, small), len(roots), len(small)


def prepare_grid(p):
    """(b)-(d) on one [m,m,m] float32 grid -> dict(status, stats [8], small
    uint8 [m,m,m], info).  info names the branch taken and holds every
    decision statistic (tests/test_unmoldref.py checks their margins)."""
    p = np.asarray(p, np.float32)
    n = p.size
    x = p.astype(np.float64).ravel()
    s = np.sort(x)
    lo, hi = s[0], s[-1]
    mean = x.sum() / n
    dv = x - mean
    std = np.sqrt((dv * dv).sum() / n)
    p50, p95 = percentile(s, 50.0), percentile(s, 95.0)
    stats = np.array([lo, hi, mean, std, p50, p95, 0.0, 0.0])
    small = np.zeros(p.shape, np.uint8)
    info = {"branch": None, "n_active": None, "density": None, "cleaned": False, "components": 0, "removed": 0,
            "decisions": {"min": lo, "max": hi, "std": std, "p95": p95}}
    if lo < -0.1 or hi > 1.1:
        return {"status": RANGE, "stats": stats, "small": small, "info": info}
    if std < 1e-6:
        return {"status": FLAT, "stats": stats, "small": small, "info": info}
    if p95 < 0.10:
        return {"status": FAINT, "stats": stats, "small": small, "info": info}
    info["decisions"]["mean"] = mean
    if mean > 0.4:
        thr, info["branch"] = 0.5, "high"
    elif mean < 0.1:
        a0 = int(np.searchsorted(s, p50, side="right"))          # active = s[a0:], the values > p50
        info["n_active"] = n - a0
        if n - a0 > 10:
            thr, info["branch"] = min(max(percentile(s[a0:], 30.0), 0.15), 0.45), "percentile"
        else:
            thr, info["branch"] = 0.30, "few_active"
    else:
        thr, info["branch"] = min(max(otsu_threshold(x, lo, hi), 0.20), 0.6), "otsu"
    resize_thr = 0.3 if mean < 0.15 else 0.4
    stats[6], stats[7] = thr, resize_thr
    b = (x >= thr).reshape(p.shape)
    density = int(b.sum()) / n
    info["density"] = density
    if density < 0.0001:
        return {"status": EMPTY, "stats": stats, "small": small, "info": info}
    if 0.0001 < density < 0.95:
        b, info["components"], info["removed"] = clean_components(b)
        info["cleaned"] = True
    return {"status": OK, "stats": stats, "small": b.astype(np.uint8), "info": info}


# ---- (e) resize -------------------------------------------------------------
def resize_axis(m, size):
    c = (np.arange(size) + 0.5) * (m / size) - 0.5
    i0 = np.floor(c)
    return i0.astype(np.int64), c - i0


def resize_values(small, size):
    """Trilinear, half-voxel centres, zero extension: float64 [hh,ww,dd]."""
    m = small.shape[0]
    P = np.zeros((m + 2,) * 3)
    P[1:-1, 1:-1, 1:-1] = small
    (y0, ty), (x0, tx), (z0, tz) = (resize_axis(m, int(v)) for v in size)
    y0, x0, z0 = y0 + 1, x0 + 1, z0 + 1                          # padded indices
    ys = np.concatenate([y0, y0 + 1])
    xs = np.concatenate([x0, x0 + 1])
    Q = P[ys][:, xs]                                             # [2hh, 2ww, m+2]
    a, b = Q[:, :, z0], Q[:, :, z0 + 1]
    vz = a + (b - a) * tz[None, None, :]
    ww = len(x0)
    a, b = vz[:, :ww], vz[:, ww:]
    vx = a + (b - a) * tx[None, :, None]
    hh = len(y0)
    a, b = vx[:hh], vx[hh:]
    return a + (b - a) * ty[:, None, None]


# ---- the whole of section 1 ------------------------------------------------
def unmold(detections, mrcnn_mask, shape):
    """detections [N,8] float32, mrcnn_mask [N,m,m,m,C] float32 probabilities ->
    dict of small [N,m^3] uint8, box_i [N,6] int32, status [N] int32, stats
    [N,8], area_pred [N] int32, dense [N,H,W,D] uint8, seg_union [H,W,D] uint8,
    infos."""
    detections = np.asarray(detections, np.float32)
    mrcnn_mask = np.asarray(mrcnn_mask, np.float32)
    N, m, C = detections.shape[0], mrcnn_mask.shape[1], mrcnn_mask.shape[-1]
    H, W, D = (int(v) for v in shape)
    out = {"small": np.zeros((N, m ** 3), np.uint8), "box_i": np.zeros((N, 6), np.int32),
           "status": np.zeros(N, np.int32), "stats": np.zeros((N, 8)), "area_pred": np.zeros(N, np.int32),
           "dense": np.zeros((N, H, W, D), np.uint8), "infos": [None] * N}
    for i in range(N):
        keep, box, cid = box_and_keep(detections[i], shape)
        if not keep:
            out["status"][i] = NOT_KEPT
            continue
        out["box_i"][i] = box
        ch = 0 if C == 1 else min(cid, C - 1)
        r = prepare_grid(mrcnn_mask[i, :, :, :, ch])
        out["status"][i], out["stats"][i], out["infos"][i] = r["status"], r["stats"], r["info"]
        out["small"][i] = r["small"].ravel()
        if r["status"] != OK:
            continue
        size = box[3:] - box[:3]
        full = resize_values(r["small"], size) >= r["stats"][7]
        area = int(full.sum())
        r["info"]["sparse_ratio"] = area / (int(size[0]) * int(size[1]) * int(size[2]))
        if r["info"]["sparse_ratio"] < 0.00001:
            out["status"][i] = SPARSE
            continue
        out["area_pred"][i] = area
        out["dense"][i, box[0]:box[3], box[1]:box[4], box[2]:box[5]] = full
    out["seg_union"] = out["dense"].any(0).astype(np.uint8)
    return out


def overlaps(dense, gt_masks):
    """dense [N,H,W,D] uint8, gt_masks [H,W,D,G] uint8 (set = non-zero) ->
    inter [N,G] int32, area_gt [G] int32."""
    g = (np.asarray(gt_masks) != 0).reshape(-1, gt_masks.shape[-1])
    d = (np.asarray(dense) != 0).reshape(dense.shape[0], -1)
    inter = d.astype(np.float64) @ g.astype(np.float64)          # counts < 2^53: exact in any order
    return inter.astype(np.int32), g.sum(0, dtype=np.int64).astype(np.int32)


def iou_matrix(inter, area_pred, area_gt):
    with np.errstate(divide="ignore", invalid="ignore"):
        i = inter.astype(np.float32)
        return i / (area_pred.astype(np.float32)[:, None] + area_gt.astype(np.float32)[None, :] - i)


def compact(detections, status, shape):
    """The reference's kept list: pixel boxes (float32), scores, class ids and
    the row indices, in detection order.  Rejected-but-kept detections stay in
    it with an all-zero mask."""
    detections = np.asarray(detections, np.float32)
    H, W, D = shape
    rows = np.flatnonzero(np.asarray(status) != NOT_KEPT)
    boxes = detections[rows, :6] * np.array([H, W, D, H, W, D], np.float32)
    return boxes, detections[rows, 7], detections[rows, 6].astype(np.int32), rows


# ---- matching and AP --------------------------------------------------------
# Written from the rule, with plain Python scalars and lists, independently of
# m3d/evaluate.py (which is vectorised): the two share no code, so
# tests/test_unmoldref.py can hold one against the other.
def _tries(row):
    """The GT indices one prediction tries, best first: a NaN IoU before any
    number, larger IoU before smaller, the later GT before the earlier at a tie."""
    def rank(j):
        v = float(row[j])
        return (1, 0.0, j) if v != v else (0, v, j)
    return sorted(range(len(row)), key=rank, reverse=True)


def compute_matches(overlaps_, pred_class_ids, gt_class_ids, iou_threshold=0.5, score_threshold=0.0):
    """Greedy matching in prediction order on the [N,G] IoU matrix ->
    (gt_match [G], pred_match [N], matched IoUs), -1 = unmatched.  Comparisons
    with a NaN IoU are false, so it is under neither threshold."""
    n_pred = len(overlaps_)
    n_gt = len(gt_class_ids)
    owner = [-1] * n_gt
    choice = [-1] * n_pred
    matched = []
    for i in range(n_pred):
        row = overlaps_[i]
        for j in _tries(row):
            if row[j] < score_threshold:
                break                                           # everything after it is cut off
            if owner[j] != -1:
                continue
            if row[j] < iou_threshold:
                break
            if int(pred_class_ids[i]) != int(gt_class_ids[j]):
                continue
            owner[j], choice[i] = i, j
            matched.append(row[j])
            break
    return np.array(owner, np.int64), np.array(choice, np.int64), matched


def _ratio(a, b):
    if b == 0:
        return float("nan") if a == 0 else float("inf")
    return a / b


def compute_ap(overlaps_, pred_class_ids, gt_class_ids, iou_threshold=0.5):
    """VOC-style AP -> (mAP, precision, recall, matched IoUs): the area under
    the precision envelope over the recall axis, recall rounded to float32."""
    _, choice, matched = compute_matches(overlaps_, pred_class_ids, gt_class_ids, iou_threshold)
    n_pred, n_gt = len(choice), len(gt_class_ids)
    curve = [(0.0, 0.0)]                                         # (recall, precision) after each prediction
    hits = 0
    for k in range(n_pred):
        hits += int(choice[k] >= 0)
        recall32 = float(np.float32(hits) / np.float32(n_gt)) if n_gt else _ratio(hits, 0)
        curve.append((recall32, hits / (k + 1)))
    curve.append((1.0, 0.0))
    area, best = 0.0, 0.0
    terms = []
    for k in range(len(curve) - 1, 0, -1):                       # from the right: best = the envelope at k
        best = max(best, curve[k][1])
        width = curve[k][0] - curve[k - 1][0]
        if width != 0:
            terms.append(width * best)
    for t in reversed(terms):
        area += t
    return area, _ratio(hits, n_pred), _ratio(hits, n_gt), matched


# ---- the committed test cases ----------------------------------------------
ROWS = ("padding", "tiny_box", "dense_high", "thin_percentile", "low_face_otsu", "high_face_few_active", "range",
        "flat", "faint", "empty", "sparse", "clean_otsu")
SHAPE = (24, 20, 16)


def _ball(m, centre, radius):
    g = np.indices((m, m, m)).astype(np.float64)
    return sum((g[a] - centre[a]) ** 2 for a in range(3)) <= radius ** 2


def case_grids(m, seed=0):
    """The 12 designed [m,m,m] float32 grids (ROWS order; rows 0 and 1 random)."""
    rng = np.random.default_rng(100 + seed + m)
    n = m ** 3
    u = lambda lo, hi: rng.uniform(lo, hi, (m, m, m))             # noqa: E731
    g = {}
    g["padding"] = u(0.0, 1.0)
    g["tiny_box"] = u(0.0, 1.0)
    # mean > 0.4; density >= 0.95, so cleaning is skipped although voxel (3,3,3) is isolated by a zero shell
    a = u(0.55, 0.95)
    for dy, dx, dz in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
        a[3 + dy, 3 + dx, 3 + dz] = 0.05
    g["dense_high"] = a
    # mean < 0.1, more than 10 values above the median: 30th percentile of the active values
    a = u(0.0, 0.02)
    a = np.where(_ball(m, (m / 2, m / 2, m / 2), m * 0.3), u(0.2, 0.9), a)
    g["thin_percentile"] = a
    # 0.1 <= mean <= 0.4: Otsu
    a = u(0.02, 0.12)
    a = np.where(_ball(m, (m * 0.4, m * 0.5, m * 0.5), m * 0.36), u(0.6, 0.95), a)
    g["low_face_otsu"] = a
    # mean < 0.1, the upper 60 % tie with the median, 8 values above it: thr = 0.30
    a = np.zeros(n)
    a[: (6 * n) // 10] = 0.12
    a = rng.permutation(a).reshape(m, m, m)
    a[3:5, 4:6, 5:7] = 0.9                                       # where a 10 x 8 x 7 target samples m = 28
    g["high_face_few_active"] = a
    a = u(0.0, 1.0)
    a[1, 2, 3] = 1.5
    g["range"] = a
    g["flat"] = np.full((m, m, m), 0.3)
    g["faint"] = u(0.0, 0.05)
    g["empty"] = u(0.41, 0.49)                                   # mean > 0.4, nothing reaches 0.5
    # three voxels on x = z = 2, which no sample of a size-3 target axis reads: area 0 after the resize
    a = np.full((m, m, m), 0.12)
    a[0:3, 2, 2] = 0.9
    g["sparse"] = a
    # Otsu; one ball plus one isolated voxel that the cleaning removes
    a = u(0.02, 0.08)
    a = np.where(_ball(m, (m * 0.5, m * 0.45, m * 0.55), m * 0.38), u(0.7, 0.9), a)
    a[0, 0, 0] = 0.85
    g["clean_otsu"] = a
    return {k: v.astype(np.float32) for k, v in g.items()}


def case_detections():
    """[12,8] float32 on SHAPE, scores descending."""
    H, W, D = SHAPE
    px = {
        "padding": (0, 0, 0, 0, 0, 0),
        "tiny_box": (3.0, 4.0, 5.0, 9.0, 4.4, 11.0),             # 0.4 voxel wide
        "dense_high": (2.0, 6.3, 3.0, 22.0, 8.6, 13.0),          # 20 x 3 x 10
        "thin_percentile": (4.2, 0.0, 5.1, 17.7, 20.0, 5.9),     # 14 x 20 x 1
        "low_face_otsu": (-3.0, -2.5, -1.0, 9.5, 10.0, 5.0),     # clipped at the low faces
        "high_face_few_active": (14.0, 12.5, 9.0, 30.0, 26.0, 20.0),   # clipped at the high faces
        "range": (1.0, 1.0, 1.0, 9.0, 9.0, 9.0),
        "flat": (2.0, 2.0, 2.0, 8.0, 8.0, 8.0),
        "faint": (3.0, 3.0, 3.0, 12.0, 12.0, 12.0),
        "empty": (5.0, 5.0, 5.0, 15.0, 15.0, 15.0),
        "sparse": (10.0, 10.0, 10.0, 13.0, 13.0, 13.0),          # 3 x 3 x 3
        "clean_otsu": (1.5, 0.0, 0.5, 19.2, 20.0, 15.0),         # 18 x 20 x 15
    }
    cls = {"padding": 0, "clean_otsu": 2}
    det = np.zeros((len(ROWS), 8), np.float32)
    for i, name in enumerate(ROWS):
        det[i, :6] = np.array(px[name], np.float64) / np.array([H, W, D, H, W, D], np.float64)
        det[i, 6] = cls.get(name, 1)
        det[i, 7] = 0.0 if name == "padding" else 0.99 - 0.05 * i
    # the padding row is last in a real DetectionLayer output; keep it first here on purpose
    return det


def case(m, C, seed=0):
    """(detections [12,8], mrcnn_mask [12,m,m,m,C]) of the committed cases."""
    grids = case_grids(m, seed)
    det = case_detections()
    rng = np.random.default_rng(7 + seed + m + C)
    mask = rng.uniform(0.0, 1.0, (len(ROWS), m, m, m, C)).astype(np.float32)
    for i, name in enumerate(ROWS):
        ch = 0 if C == 1 else min(int(det[i, 6]), C - 1)
        mask[i, :, :, :, ch] = grids[name]
    return det, mask


def case_gt(G, shape=SHAPE, seed=0):
    """[H,W,D,G] uint8: overlapping boxes and balls; the last mask (G > 1) is all zero."""
    rng = np.random.default_rng(50 + seed + G)
    H, W, D = shape
    gt = np.zeros((H, W, D, G), np.uint8)
    for k in range(G):
        if G > 1 and k == G - 1:
            continue
        lo = np.array([rng.integers(0, s // 2) for s in shape])
        hi = np.array([rng.integers(l + 2, s + 1) for l, s in zip(lo, shape)])
        gt[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2], k] = 1
        if k % 2:
            gt[..., k] &= (rng.uniform(size=shape) < 0.7).astype(np.uint8)
    return gt
