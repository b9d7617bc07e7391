"""The stored head targets on the host (m3d.headstore's file layout,
m3d.dataset.ToyHeadDataset, m3d.generator.select_head_rois): the reference's
.npz keys and dtypes (core/models.py:3604-3636) round-tripped through the
reader (core/data_generators.py:1873-2023), and the ROI selection of
HeadGenerator.__getitem__ (492-640) checked by its properties.  No GPU."""
import csv
import os
import types

import numpy as np
import pytest

T_ROIS = 5


@pytest.fixture(scope="module")
def stored(tmp_path_factory):
    """Two images written through the host-array writer; image 1 has one positive."""
    from m3d import headstore
    root = str(tmp_path_factory.mktemp("headstore"))
    rng = np.random.default_rng(3)
    csv_path = headstore.write_csv_header(root, "train")
    images = []
    for i, name in enumerate(("vol_a", "vol_b")):
        a = {"rois": rng.uniform(0, 1, (T_ROIS, 6)).astype(np.float32),
             "rois_aligned": rng.normal(size=(T_ROIS, 2, 2, 2, 4)).astype(np.float32),
             "mask_aligned": rng.uniform(0, 1, (T_ROIS, 3, 3, 3, 4)).astype(np.float32),     # 5-D
             "tci": np.array([[1, 0, 1, 1, 0], [0, 0, 1, 0, 0]][i], np.int32),
             "bbox": rng.normal(size=(T_ROIS, 6)).astype(np.float32),
             "target_mask": (rng.uniform(0, 1, (T_ROIS, 4, 4, 4)) > 0.6).astype(np.float32)}  # 4-D
        paths = headstore.save_head_target_arrays(
            root, name, a["rois"], a["rois_aligned"].astype(np.float16), np.packbits(a["mask_aligned"] > 0.5),
            a["mask_aligned"].shape, a["tci"], a["bbox"], np.packbits(a["target_mask"] > 0.5), a["target_mask"].shape)
        headstore.append_csv_row(csv_path, paths)
        images.append((name, a, paths))
    return root, csv_path, images


def test_file_layout_keys_and_dtypes(stored):
    from m3d import headstore
    root, csv_path, images = stored
    assert headstore.COLUMNS == ("rois", "rois_aligned", "mask_aligned", "target_class_ids", "target_bbox",
                                 "target_mask")
    want = {"rois": {"rois": np.float32}, "rois_aligned": {"rois_aligned": np.float16},
            "mask_aligned": {"mask_bits": np.uint8, "mask_shape": np.int32}, "target_class_ids": {"tci": np.int32},
            "target_bbox": {"bbox": np.float32}, "target_mask": {"tm_bits": np.uint8, "tm_shape": np.int32}}
    for name, a, paths in images:
        assert paths == tuple(os.path.join(root, col, name + ".npz") for col in headstore.COLUMNS)
        for col, path in zip(headstore.COLUMNS, paths):
            with np.load(path, allow_pickle=False) as z:
                assert {k: z[k].dtype.type for k in z.files} == want[col], col
        with np.load(paths[2]) as z:
            assert z["mask_shape"].tolist() == [T_ROIS, 3, 3, 3, 4] and z["mask_bits"].ndim == 1
            assert z["mask_bits"].size == (T_ROIS * 27 * 4 + 7) // 8
        with np.load(paths[5]) as z:
            assert z["tm_shape"].tolist() == [T_ROIS, 4, 4, 4] and z["tm_bits"].size == T_ROIS * 64 // 8
    assert csv_path == os.path.join(root, "datasets", "train.csv")
    with open(csv_path, newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == list(headstore.COLUMNS)
    assert rows[1:] == [list(paths) for _, _, paths in images]


def test_round_trip_through_the_dataset(stored):
    from m3d.dataset import ToyHeadDataset
    root, _, images = stored
    ds = ToyHeadDataset()
    ds.load_dataset(root, is_train=True)
    ds.prepare()
    assert list(ds.image_ids) == [0, 1] and ds.num_classes == 2
    for image_id, (name, a, _) in enumerate(images):
        assert ds.image_info[image_id]["path"] == name + ".npz"
        rois, ra, ma, tci, tb, tm = ds.load_data(image_id)
        assert [x.dtype for x in (rois, ra, ma, tci, tb, tm)] == [np.float32, np.float32, np.float32, np.int32,
                                                                  np.float32, np.float32]
        assert np.array_equal(rois, a["rois"]) and np.array_equal(tci, a["tci"]) and np.array_equal(tb, a["bbox"])
        assert np.array_equal(ra, a["rois_aligned"].astype(np.float16).astype(np.float32))
        assert ma.shape == (T_ROIS, 3, 3, 3, 4) and np.array_equal(ma, (a["mask_aligned"] > 0.5).astype(np.float32))
        assert tm.shape == (T_ROIS, 4, 4, 4, 1)                     # the trailing channel axis of a 4-D mask
        assert np.array_equal(tm[..., 0], a["target_mask"])


def test_plain_npy_and_column_names(stored, tmp_path):
    """Column names match case-insensitively and by the reference's
    alternatives; a plain .npy is read as well as an .npz; a missing optional
    column is zeros of the configuration's shape."""
    from m3d.dataset import ToyHeadDataset
    _, _, images = stored
    a = images[0][1]
    os.makedirs(tmp_path / "datasets")
    for k in ("rois", "rois_aligned", "tci", "mask_aligned"):
        np.save(tmp_path / (k + ".npy"), a[k])
    with open(tmp_path / "datasets" / "test.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["ROIS", "Rois_Aligned", "tci_path", "MASK_ALIGNED"])
        w.writerow([str(tmp_path / (k + ".npy")) for k in ("rois", "rois_aligned", "tci", "mask_aligned")])
    cfg = types.SimpleNamespace(NUM_CLASSES=2, MASK_SHAPE=[6, 6, 6], MASK_POOL_SIZE=3, TOP_DOWN_PYRAMID_SIZE=4)
    ds = ToyHeadDataset(config=cfg)
    ds.load_dataset(str(tmp_path), is_train=False)
    ds.prepare()
    rois, ra, ma, tci, tb, tm = ds.load_data(0)
    assert np.array_equal(rois, a["rois"]) and np.array_equal(ra, a["rois_aligned"]) and np.array_equal(tci, a["tci"])
    assert np.array_equal(ma, a["mask_aligned"])
    assert tb.shape == (T_ROIS, 6) and not tb.any() and tm.shape == (T_ROIS, 6, 6, 6, 1) and not tm.any()
    with open(tmp_path / "datasets" / "train.csv", "w", newline="") as f:
        csv.writer(f).writerow(["rois", "target_class_ids"])
    with pytest.raises(KeyError, match="rois_aligned"):
        ToyHeadDataset().load_dataset(str(tmp_path), is_train=True)


def test_filter_by_positive_count(stored):
    from m3d.dataset import ToyHeadDataset
    root = stored[0]
    ds = ToyHeadDataset()
    ds.load_dataset(root)
    ds.prepare()
    assert ds.filter_by_positive_count(1) == [] and list(ds.image_ids) == [0, 1]
    assert ds.filter_by_positive_count(2) == [("vol_b.npz", 1)] and list(ds.image_ids) == [0]
    assert ds.filter_by_positive_count(4) == [("vol_a.npz", 3)] and len(ds.image_ids) == 0


# --------------------------------------------------------------------------- the selection
def _cfg(**kw):
    return types.SimpleNamespace(**kw)


def _sel(tci, cov, T, seed=0, training=True, **kw):
    from m3d.generator import select_head_rois
    return select_head_rois(np.asarray(tci, np.int32), np.asarray(cov, np.float32), T, _cfg(**kw),
                            np.random.RandomState(seed), training)


def test_selection_keeps_everything_when_it_fits():
    tci = [1, 0, 0, 2, 0]
    sel = _sel(tci, np.zeros(5), 8, seed=4)
    assert sel.dtype == np.int64 and sel.shape == (8,)
    assert sorted(sel[:5]) == [0, 1, 2, 3, 4] and list(sel[5:]) == [-1, -1, -1]
    assert list(sel[:5]) != [0, 1, 2, 3, 4]                         # HEAD_SHUFFLE_ROIS defaults to True (seed 4 moves it)
    assert list(_sel(tci, np.zeros(5), 8, HEAD_SHUFFLE_ROIS=False)) == [0, 1, 2, 3, 4, -1, -1, -1]
    assert list(_sel(tci, np.zeros(5), 5, HEAD_SHUFFLE_ROIS=False)) == [0, 1, 2, 3, 4]
    assert list(_sel([], [], 3)) == [-1, -1, -1]


def test_selection_balances_and_prefers_strong_positives():
    rng = np.random.default_rng(0)
    tci = np.array([1] * 20 + [0] * 40)
    cov = np.concatenate([np.full(10, 0.01), np.full(10, 0.5), np.zeros(40)])    # positives 0..9 weak, 10..19 strong
    perm = rng.permutation(60)
    tci, cov = tci[perm], cov[perm]
    T = 12
    for frac in (0.33, 0.5):
        sel = _sel(tci, cov, T, HEAD_POS_FRAC=frac)
        assert sel.shape == (T,) and sel.min() >= 0 and len(set(sel)) == T          # enough of both: no repeats
        pos = sel[tci[sel] > 0]
        assert len(pos) == int(round(T * frac))
        assert (cov[pos] >= 0.06).all()                                             # no weak one while strong ones exist
    # the threshold is the configuration's
    sel = _sel(tci, cov, T, HEAD_MIN_POSITIVE_COVERAGE=0.005, HEAD_POS_FRAC=1.0, seed=1)
    assert (tci[sel] > 0).all()
    seen = set()
    for seed in range(8):
        s = _sel(tci, cov, T, HEAD_MIN_POSITIVE_COVERAGE=0.005, HEAD_POS_FRAC=1.0, seed=seed)
        seen |= set(np.asarray(cov)[s].round(3).tolist())
    assert seen == {0.01, 0.5}


def test_selection_all_weak_takes_the_best():
    tci = np.array([1] * 9 + [0] * 30)
    cov = np.concatenate([np.linspace(0.001, 0.009, 9), np.zeros(30)]).astype(np.float32)
    for T, n_best in ((8, 4), (30, 9), (1, 1)):
        assert n_best == min(9, max(1, T // 2))
        best = set(np.argsort(cov[:9])[::-1][:n_best].tolist())
        sel = _sel(tci, cov, T, HEAD_POS_FRAC=1.0)                  # every slot may go to a positive
        pos = set(sel[tci[sel] > 0].tolist())
        assert pos == best and len(sel) == T, (T, pos, best)


def test_selection_one_kind_only_and_top_up():
    # no negatives: all positives; with replacement only when short
    tci, cov = np.ones(10, np.int32), np.full(10, 0.5)
    sel = _sel(tci, cov, 6)
    assert len(set(sel)) == 6 and sel.min() >= 0
    tci, cov = np.array([1] * 3 + [0] * 7), np.array([0.5] * 3 + [0.0] * 7)
    sel = _sel(tci, cov, 8, HEAD_POS_FRAC=0.5)                       # 3 positives for 4 slots: negatives top up
    assert sorted(sel[tci[sel] > 0]) == [0, 1, 2] and len(set(sel)) == 8
    tci, cov = np.array([1] * 9 + [0] * 2), np.array([0.5] * 9 + [0.0] * 2)
    sel = _sel(tci, cov, 8, HEAD_POS_FRAC=0.25)                      # 2 negatives for 6 slots: positives top up
    assert sorted(sel[tci[sel] == 0]) == [9, 10] and len(set(sel)) == 8
    # the mirror case: no positives
    sel = _sel(np.zeros(10, np.int32), np.zeros(10), 6)
    assert len(set(sel)) == 6 and sel.min() >= 0
    # more rows than T but one side short of T: strong positives only, so draws repeat
    tci, cov = np.ones(10, np.int32), np.array([0.5] * 4 + [0.01] * 6)
    sel = _sel(tci, cov, 6)
    assert set(sel) <= {0, 1, 2, 3} and len(sel) == 6


def test_selection_is_seeded_and_plain_without_training():
    rng = np.random.default_rng(1)
    tci = (rng.uniform(size=40) < 0.4).astype(np.int32)
    cov = rng.uniform(0, 0.3, 40).astype(np.float32)
    a, b, c = _sel(tci, cov, 16, seed=7), _sel(tci, cov, 16, seed=7), _sel(tci, cov, 16, seed=8)
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    # training=False: no shuffle, no balancing -- the identity order while it fits ...
    assert list(_sel(tci[:10], cov[:10], 12, training=False)) == list(range(10)) + [-1, -1]
    # ... and a plain draw without replacement (never the coverages) when it does not
    from m3d.generator import select_head_rois

    def never(rows):
        raise AssertionError("coverage is not read outside the balanced branch")
    sel = select_head_rois(tci, never, 16, _cfg(), np.random.RandomState(0), training=False)
    assert len(set(sel)) == 16 and sel.min() >= 0
    sel = select_head_rois(tci, never, 16, _cfg(HEAD_BALANCE_POS=False), np.random.RandomState(0), training=True)
    assert len(set(sel)) == 16
    want = np.random.RandomState(0)
    order = np.arange(40, dtype=np.int32)
    want.shuffle(order)
    assert np.array_equal(sel, want.choice(order, size=16, replace=False))      # the reference's call order


def test_index_tables():
    from m3d.headstore import index_table
    assert index_table(4, 3).tolist() == [0, 1, 3] and index_table(4, 3).dtype == np.int64
    assert index_table(3, 4).tolist() == [0, 0, 1, 2]
    assert index_table(5, 5).tolist() == [0, 1, 2, 3, 4]
    for s, m in ((4, 3), (3, 4), (14, 28), (28, 14), (7, 7), (1, 3)):
        want = np.arange(s) if s == m else np.linspace(0, s - 1, m).astype(np.int64)
        assert np.array_equal(index_table(s, m), want)
