"""Pins tests/unmoldref.py, the numpy float64 restatement of detection unmolding
and mask-IoU evaluation that tests/test_gpu_unmold.py compares the kernels of
csrc/unmold.hip with: hand-derived known answers, cross-checks with
scipy.ndimage (zoom, label) and np.histogram, hand-worked matching / AP cases,
and two conditions on the committed test cases themselves -- they reach every
branch, and every decision statistic lies at least 1e-6 from its constant, so
the GPU's reduction order cannot flip a branch."""
import functools

import numpy as np
import pytest

import unmoldref as U


# ---- hand-derived known answers --------------------------------------------
def test_resize_2_to_4_zero_border_by_hand():
    """m = 2 -> 4: c = -0.25, 0.25, 0.75, 1.25.  For a row (a, b) the samples
    are 0.75 a, a + 0.25 (b - a), a + 0.75 (b - a), 0.75 b: the outer two blend
    with the zero border."""
    i0, t = U.resize_axis(2, 4)
    assert i0.tolist() == [-1, 0, 0, 1] and t.tolist() == [0.75, 0.25, 0.75, 0.25]
    w = np.array([0.75, 1.0, 1.0, 0.75])
    ones = U.resize_values(np.ones((2, 2, 2), np.uint8), (4, 4, 4))
    assert np.array_equal(ones, w[:, None, None] * w[None, :, None] * w[None, None, :])
    one = np.zeros((2, 2, 2), np.uint8)
    one[0, 0, 0] = 1
    v = np.array([0.75, 0.75, 0.25, 0.0])
    assert np.array_equal(U.resize_values(one, (4, 4, 4)), v[:, None, None] * v[None, :, None] * v[None, None, :])
    # anisotropic: a = 1, b = 0 along z only, constant 1 along y and x (m = 2 -> 4, 2, 4)
    g = np.zeros((2, 2, 2), np.uint8)
    g[:, :, 0] = 1
    got = U.resize_values(g, (4, 2, 4))
    wy, wx = np.array([0.75, 1.0, 1.0, 0.75]), np.array([1.0, 1.0])
    assert np.array_equal(got, wy[:, None, None] * wx[None, :, None] * v[None, None, :])


def test_resize_identity():
    rng = np.random.default_rng(0)
    g = (rng.uniform(size=(7, 7, 7)) < 0.4).astype(np.uint8)
    assert np.array_equal(U.resize_values(g, (7, 7, 7)), g.astype(np.float64))


def test_resize_single_voxel():
    g = np.zeros((8, 8, 8), np.uint8)
    g[2, 2, 2] = 1
    p = np.zeros(16)
    p[3:7] = [0.25, 0.75, 0.75, 0.25]                           # c = 1.25, 1.75, 2.25, 2.75
    assert np.array_equal(U.resize_values(g, (16, 16, 16)), p[:, None, None] * p[None, :, None] * p[None, None, :])
    # a size-3 axis samples c = 5/6, 3.5, 37/6: index 2 is never read
    assert not U.resize_values(g, (3, 3, 3)).any()


def test_box_clipped_at_each_face():
    H, W, D = 24, 20, 16
    sc = np.array([H, W, D, H, W, D], np.float64)

    def box(px, cid=1):
        d = np.zeros(8, np.float32)
        d[:6] = np.array(px) / sc
        d[6] = cid
        return U.box_and_keep(d, (H, W, D))

    keep, b, cid = box((2.25, 3.5, 4.75, 10.5, 11.25, 12.0))
    assert keep and cid == 1 and b.tolist() == [2, 3, 4, 11, 12, 12]
    assert box((-3.0, 3.0, 4.0, 5.0, 6.0, 7.0))[1].tolist() == [0, 3, 4, 5, 6, 7]          # y low
    assert box((3.0, -0.5, 4.0, 5.0, 6.0, 7.0))[1].tolist() == [3, 0, 4, 5, 6, 7]          # x low
    assert box((3.0, 3.0, -9.0, 5.0, 6.0, 7.0))[1].tolist() == [3, 3, 0, 5, 6, 7]          # z low
    assert box((3.0, 3.0, 4.0, 30.0, 6.0, 7.0))[1].tolist() == [3, 3, 4, 24, 6, 7]         # y high
    assert box((3.0, 3.0, 4.0, 5.0, 20.5, 7.0))[1].tolist() == [3, 3, 4, 5, 20, 7]         # x high
    assert box((3.0, 3.0, 4.0, 5.0, 6.0, 99.0))[1].tolist() == [3, 3, 4, 5, 6, 16]         # z high
    assert box((30.0, 3.0, 4.0, 40.0, 6.0, 7.0))[1].tolist() == [23, 3, 4, 24, 6, 7]       # wholly outside: 1 voxel
    assert not box((2.0, 3.0, 4.0, 10.0, 11.0, 12.0), cid=0)[0]
    assert not box((2.0, 3.0, 4.0, 10.0, 3.25, 12.0))[0]                                   # 0.25 voxel wide
    assert box((2.0, 3.0, 4.0, 10.0, 3.75, 12.0))[0]                                       # 0.75 voxel wide


def test_percentile_of_a_ramp():
    s = np.arange(11, dtype=np.float64)
    assert U.percentile(s, 50.0) == 5.0 and U.percentile(s, 95.0) == 9.5 and U.percentile(s, 30.0) == 3.0
    assert U.percentile(np.arange(4.0), 50.0) == 1.5
    assert U.percentile(np.array([2.5]), 95.0) == 2.5
    rng = np.random.default_rng(1)
    x = np.sort(rng.uniform(size=513))
    for q in (30.0, 50.0, 95.0):
        assert abs(U.percentile(x, q) - np.percentile(x, q)) < 1e-14


def test_otsu_of_a_two_valued_grid():
    """Two populated bins (0 and 255): the between-class variance is the same
    for every split between them, the first wins: centers[0] = lo + bw / 2."""
    x = np.array([0.25] * 300 + [0.75] * 212)
    assert U.otsu_threshold(x, 0.25, 0.75) == 0.25 + 0.5 * (0.5 / 256.0)
    p = np.full((8, 8, 8), 0.25, np.float32)
    p[:3] = 0.75
    r = U.prepare_grid(p)                                       # mean 0.4375 > 0.4: the 0.5 branch instead
    assert r["info"]["branch"] == "high" and r["stats"][6] == 0.5
    p[2:] = 0.25                                                # mean 0.375: Otsu, clipped to [0.2, 0.6]
    r = U.prepare_grid(p)
    assert r["info"]["branch"] == "otsu" and r["stats"][6] == 0.25 + 0.5 * (0.5 / 256.0)
    assert r["status"] == U.OK and np.array_equal(r["small"], (p == 0.75).astype(np.uint8))


# ---- cross-checks -----------------------------------------------------------
@pytest.mark.parametrize("size", [(37, 19, 9), (5, 3, 1), (200, 2, 3), (1, 1, 1), (8, 8, 8), (11, 30, 4)])
def test_resize_against_scipy_zoom(size):
    import scipy.ndimage as ndi
    rng = np.random.default_rng(sum(size))
    g = (rng.uniform(size=(8, 8, 8)) < 0.5).astype(np.uint8)
    want = ndi.zoom(g.astype(np.float64), [s / 8 for s in size], order=1, mode="grid-constant", cval=0.0,
                    grid_mode=True)
    got = U.resize_values(g, size)
    assert want.shape == tuple(size)
    assert np.abs(got - want).max() < 1e-9
    for thr in (0.3, 0.4):
        if np.abs(got - thr).min() > 1e-6:                      # no tie at the threshold: the masks agree
            assert np.array_equal(got >= thr, want >= thr)


def test_cleaning_against_scipy_label():
    import scipy.ndimage as ndi
    rng = np.random.default_rng(5)
    for m, dens in ((8, 0.2), (8, 0.5), (13, 0.25), (28, 0.12)):
        b = rng.uniform(size=(m, m, m)) < dens
        lab, k = ndi.label(b)                                   # default structure: 6-neighbour
        mine = U.label_min(b)
        assert len(np.unique(mine[b])) == k
        for c in range(1, k + 1):                               # same partition; the label is the smallest flat index
            idx = np.flatnonzero(lab.ravel() == c)
            assert (mine.ravel()[idx] == idx.min()).all()
        cleaned, ncomp, removed = U.clean_components(b)
        sizes = np.bincount(lab.ravel())[1:]
        min_size = max(2, int(m ** 3 * 0.0002))
        keep = np.isin(lab, 1 + np.flatnonzero(sizes >= min_size))
        assert ncomp == k and removed == int((sizes < min_size).sum()) and removed > 0
        assert np.array_equal(cleaned, keep)
    one = np.zeros((8, 8, 8), bool)
    one[4, 4, 4] = True                                         # a single component is never dropped
    assert np.array_equal(U.clean_components(one)[0], one)


def test_otsu_against_np_histogram():
    for m in (8, 28):
        x = U.case_grids(m)["low_face_otsu"].astype(np.float64).ravel()
        lo, hi = x.min(), x.max()
        counts, edges = np.histogram(x, bins=256, range=(lo, hi))
        centers = (edges[:-1] + edges[1:]) / 2
        w1 = np.cumsum(counts)
        w2 = np.cumsum(counts[::-1])[::-1]
        m1 = np.cumsum(counts * centers) / w1
        m2 = (np.cumsum((counts * centers)[::-1]) / w2[::-1])[::-1]
        want = centers[np.argmax(w1[:-1] * w2[1:] * (m1[:-1] - m2[1:]) ** 2)]
        assert abs(U.otsu_threshold(x, lo, hi) - want) <= (hi - lo) / 256
        assert np.array_equal(np.bincount(U.otsu_bins(x, lo, hi), minlength=256), counts)


# ---- matching and AP --------------------------------------------------------
def test_matches_and_ap_by_hand():
    # a perfect match
    ov = np.array([[0.9, 0.0], [0.1, 0.8]], np.float32)
    gm, pm, ious = U.compute_matches(ov, [1, 2], [1, 2])
    assert gm.tolist() == [0, 1] and pm.tolist() == [0, 1] and ious == [ov[0, 0], ov[1, 1]]
    assert U.compute_ap(ov, [1, 2], [1, 2])[:3] == (1.0, 1.0, 1.0)
    # a class mismatch: prediction 0 overlaps GT 0 but names another class
    gm, pm, _ = U.compute_matches(ov, [2, 2], [1, 2])
    assert gm.tolist() == [-1, 1] and pm.tolist() == [-1, 1]
    mAP, prec, rec, _ = U.compute_ap(ov, [2, 2], [1, 2])
    # precisions (0, .5) -> padded, made monotone: (.5, .5, .5, 0); recalls (0, 0, .5, 1): AP = .5 * .5
    assert (mAP, prec, rec) == (0.25, 0.5, 0.5)
    # two predictions compete for one GT: the first (higher score) takes it
    ov = np.array([[0.7], [0.9]], np.float32)
    gm, pm, ious = U.compute_matches(ov, [1, 1], [1])
    assert gm.tolist() == [0] and pm.tolist() == [0, -1] and ious == [ov[0, 0]]
    mAP, prec, rec, _ = U.compute_ap(ov, [1, 1], [1])
    assert (mAP, prec, rec) == (1.0, 0.5, 1.0)
    # no predictions
    mAP, prec, rec, ious = U.compute_ap(np.zeros((0, 2), np.float32), [], [1, 1])
    assert mAP == 0.0 and rec == 0.0 and np.isnan(prec) and ious == []
    # IoU exactly at the threshold matches (the test is `<`); just below does not
    ov = np.array([[0.5]], np.float32)
    assert U.compute_matches(ov, [1], [1])[1].tolist() == [0]
    assert U.compute_matches(np.array([[np.nextafter(np.float32(0.5), np.float32(0))]]), [1], [1])[1].tolist() == [-1]
    assert U.compute_matches(ov, [1], [1], iou_threshold=0.75)[1].tolist() == [-1]
    # an undefined IoU (empty prediction, empty GT) is tried first and is under neither threshold
    assert U.compute_matches(np.array([[np.nan, 0.9]], np.float32), [1], [1, 1])[1].tolist() == [0]
    # equal IoUs: the later GT is tried first; the second prediction gets the other one
    gm, pm, _ = U.compute_matches(np.array([[0.8, 0.8], [0.8, 0.8]], np.float32), [1, 1], [1, 1])
    assert pm.tolist() == [1, 0] and gm.tolist() == [1, 0]
    # a GT of another class is passed over, not a stop: the next one above the threshold matches
    assert U.compute_matches(np.array([[0.9, 0.6]], np.float32), [2], [1, 2])[1].tolist() == [1]


def test_package_matching_equals_the_restatement():
    from m3d import evaluate as E
    rng = np.random.default_rng(3)
    for trial in range(200):
        n, g = rng.integers(0, 12), rng.integers(1, 9)
        ov = rng.uniform(size=(n, g)).astype(np.float32)
        if trial % 2:
            ov = np.round(ov, 1)                                # ties, exact 0.5s and 0s
        for _ in range(trial % 4):
            if n:
                ov[rng.integers(0, n), rng.integers(0, g)] = np.nan
        pc, gc = rng.integers(1, 3, n), rng.integers(1, 3, g)
        a, b = E.compute_ap(ov, pc, gc), U.compute_ap(ov, pc, gc)
        assert np.array_equal(np.array(a[:3]), np.array(b[:3]), equal_nan=True)
        assert np.array_equal(np.array(a[3]), np.array(b[3]), equal_nan=True)
        for x, y in zip(E.compute_matches(ov, pc, gc)[:2], U.compute_matches(ov, pc, gc)[:2]):
            assert np.array_equal(x, y)
    assert (E.OK, E.NOT_KEPT, E.RANGE, E.FLAT, E.FAINT, E.EMPTY, E.SPARSE) == \
        (U.OK, U.NOT_KEPT, U.RANGE, U.FLAT, U.FAINT, U.EMPTY, U.SPARSE)


def test_iou_matrix():
    inter = np.array([[2, 0], [0, 0]], np.int32)
    iou = U.iou_matrix(inter, np.array([4, 0], np.int32), np.array([6, 0], np.int32))
    assert iou.dtype == np.float32
    assert iou[0, 0] == np.float32(2) / np.float32(8) and iou[0, 1] == 0.0 and iou[1, 0] == 0.0 and np.isnan(iou[1, 1])


# ---- the committed cases ----------------------------------------------------
@functools.lru_cache(maxsize=None)
def _unmolded(m, C):
    det, mask = U.case(m, C)
    return U.unmold(det, mask, U.SHAPE)


@pytest.mark.parametrize("m,C", [(8, 2), (8, 1), (28, 2)])
def test_cases_reach_every_branch(m, C):
    r = _unmolded(m, C)
    st = dict(zip(U.ROWS, r["status"].tolist()))
    info = dict(zip(U.ROWS, r["infos"]))
    assert st == {"padding": U.NOT_KEPT, "tiny_box": U.NOT_KEPT, "dense_high": U.OK, "thin_percentile": U.OK,
                  "low_face_otsu": U.OK, "high_face_few_active": U.OK, "range": U.RANGE, "flat": U.FLAT,
                  "faint": U.FAINT, "empty": U.EMPTY, "sparse": U.SPARSE, "clean_otsu": U.OK}
    assert {i["branch"] for i in r["infos"] if i} >= {"high", "percentile", "few_active", "otsu"}
    assert info["thin_percentile"]["branch"] == "percentile" and info["thin_percentile"]["n_active"] > 10
    assert info["high_face_few_active"]["branch"] == "few_active" and info["high_face_few_active"]["n_active"] <= 10
    assert info["clean_otsu"]["branch"] == "otsu" and info["clean_otsu"]["removed"] >= 1
    # cleaning skipped at density >= 0.95 although a one-voxel component is there
    d = info["dense_high"]
    assert d["density"] >= 0.95 and not d["cleaned"]
    g = r["small"][U.ROWS.index("dense_high")].reshape(m, m, m)
    assert g[3, 3, 3] == 1 and U.clean_components(g.astype(bool))[2] >= 1
    # both resize thresholds
    rt = {float(v) for v, s in zip(r["stats"][:, 7], r["status"]) if s in (U.OK, U.SPARSE)}
    assert rt == {0.3, 0.4}
    # boxes: thin, clipped low / high, a multiple of 5 on every axis somewhere
    b = dict(zip(U.ROWS, r["box_i"].tolist()))
    assert b["thin_percentile"][5] - b["thin_percentile"][2] == 1
    assert b["low_face_otsu"][:3] == [0, 0, 0] and b["high_face_few_active"][3:] == list(U.SHAPE)
    sizes = np.array([[v[3] - v[0], v[4] - v[1], v[5] - v[2]] for v in b.values()])
    ok = r["status"] == U.OK
    assert ((sizes[ok] % 5 == 0) & (sizes[ok] > 0)).any(0).all()
    assert (sizes[ok] > m).any() or m == 28                     # larger than m on one axis, smaller on another
    assert r["area_pred"][ok].min() > 0 and r["seg_union"].any()


@pytest.mark.parametrize("m,C", [(8, 2), (8, 1), (28, 2)])
def test_case_decisions_keep_their_margins(m, C):
    """Every decision statistic at least 1e-6 from its constant."""
    r = _unmolded(m, C)
    checked = 0
    for info in r["infos"]:
        if info is None:
            continue
        d = info["decisions"]
        pairs = [(d["min"], -0.1), (d["max"], 1.1), (d["std"], 1e-6), (d["p95"], 0.10)]
        if "mean" in d:
            pairs += [(d["mean"], 0.4), (d["mean"], 0.1), (d["mean"], 0.15)]
        if info["density"] is not None:
            pairs += [(info["density"], 0.0001), (info["density"], 0.95)]
        if "sparse_ratio" in info:
            pairs += [(info["sparse_ratio"], 0.00001)]
        for v, c in pairs:
            assert abs(v - c) >= 1e-6, (v, c)
            checked += 1
    assert checked >= 60
