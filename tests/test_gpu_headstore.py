"""The stored head targets on the GPU (csrc/headstore.hip, m3d.headstore,
MaskRCNN.head_target_generation, m3d.generator.HeadGenerator,
MaskRCNN.train_heads_on_features).  numpy's own packbits / unpackbits /
astype(np.float16) are the oracle (they are what the reference calls), and
every comparison is exact.  Each kernel call writes into the middle of a
larger buffer whose guard bands must stay intact, and runs twice."""
import bz2
import csv
import os
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BAND = 256              # guard bytes on each side of an output (keeps the 16-byte alignment)
FILL = 0xA5


# --------------------------------------------------------------------------- helpers
class Banded:
    """nbytes of device output between two guard bands."""

    def __init__(self, nbytes, cuda):
        self.nbytes = int(nbytes)
        self.buf = torch.full((self.nbytes + 2 * BAND,), FILL, dtype=torch.uint8, device=cuda)
        self.ptr = self.buf.data_ptr() + BAND

    def result(self, dtype):
        torch.cuda.synchronize()
        host = self.buf.cpu().numpy()
        assert (host[:BAND] == FILL).all() and (host[BAND + self.nbytes:] == FILL).all(), "guard band overwritten"
        return host[BAND:BAND + self.nbytes].copy().view(dtype)


def twice(call, nbytes, dtype, cuda):
    """Run ``call(out_ptr)`` into two banded buffers; the runs must agree bit for bit."""
    outs = []
    for _ in range(2):
        b = Banded(nbytes, cuda)
        call(b.ptr)
        outs.append(b.result(dtype))
    assert np.array_equal(outs[0].view(np.uint8), outs[1].view(np.uint8)), "two runs differ"
    return outs[0]


def _L():
    from m3d import _lib
    return _lib, _lib.load()


# --------------------------------------------------------------------------- pack
SPECIAL = np.array([0.5, np.nextafter(np.float32(0.5), np.float32(1)), np.nan, np.inf, -np.inf, -1.5, -0.0, 0.0,
                    np.nextafter(np.float32(0.5), np.float32(0)), 1.0, 0.75, -np.nan], np.float32)


def _pack_input(n, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(0.5, 0.5, n).astype(np.float32)
    k = min(n, len(SPECIAL))
    x[:k] = np.roll(SPECIAL, -(n % len(SPECIAL)))[:k]         # n = 1 gets a different special than n = 7
    if n > 64:
        x[-len(SPECIAL):] = SPECIAL                            # and the tail (the last, partial byte)
    return x


@pytest.mark.parametrize("n", [1, 7, 8, 9, 63, 64, 65, 8 * 256 * 3 + 5])
def test_pack_bits_is_numpy_packbits(cuda, n):
    lib, L = _L()
    x = _pack_input(n, n)
    with np.errstate(invalid="ignore"):
        want = np.packbits(x > 0.5)
    d = torch.from_numpy(x).to(cuda)
    got = twice(lambda out: lib.check(L.m3d_pack_bits_f32(d.data_ptr(), n, out, lib.stream()), "pack"),
                (n + 7) // 8, np.uint8, cuda)
    assert got.shape == want.shape and np.array_equal(got, want)
    if n % 8:
        assert got[-1] & ((1 << (8 - n % 8)) - 1) == 0         # zero-filled


def test_pack_bits_of_a_tensor(cuda):
    from m3d import headstore
    x = _pack_input(3 * 2 * 2 * 2 * 8, 11).reshape(3, 2, 2, 2, 8)
    with np.errstate(invalid="ignore"):
        want = np.packbits(x > 0.5)
    got = headstore.pack_bits(torch.from_numpy(x).to(cuda))
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    strided = torch.from_numpy(x).to(cuda).permute(4, 0, 1, 2, 3)           # packed in logical order
    with np.errstate(invalid="ignore"):
        assert np.array_equal(headstore.pack_bits(strided).cpu().numpy(), np.packbits(x.transpose(4, 0, 1, 2, 3) > 0.5))


# --------------------------------------------------------------------------- half
def _half_input():
    e = np.float32(2.0) ** -11
    sp = [1 + e, 1 + 3 * e, 65504.0, 65519.996, 65520.0, -65520.0, 1e30, -1e30, np.inf, -np.inf, np.nan,
          2.0 ** -25, np.nextafter(np.float32(2.0 ** -25), np.float32(1)), -(2.0 ** -25), 0.0, -0.0,
          2.0 ** -14, np.nextafter(np.float32(2.0 ** -14), np.float32(0)), 1e-40, -1e-40]
    sp += [k * 2.0 ** -24 for k in range(5)] + [(k + 0.5) * 2.0 ** -24 for k in range(5)]
    rng = np.random.default_rng(5)
    rand = (rng.normal(size=4096) * 10.0 ** rng.uniform(-9, 5, 4096)).astype(np.float32)
    return np.concatenate([np.array(sp, np.float32), rand, np.array([3.0], np.float32)])    # n % 4 == 3


def test_f32_to_f16_is_numpy_astype(cuda):
    lib, L = _L()
    x = _half_input()
    n = x.size
    assert n % 4 != 0
    with np.errstate(over="ignore"):
        want = x.astype(np.float16)
    d = torch.from_numpy(x).to(cuda)
    got = twice(lambda out: lib.check(L.m3d_f32_to_f16(d.data_ptr(), n, out, lib.stream()), "half"), 2 * n,
                np.uint16, cuda)
    nan = np.isnan(x)
    assert nan.any() and np.isnan(got.view(np.float16)[nan]).all()
    assert np.array_equal(got[~nan], want.view(np.uint16)[~nan])
    # the named cases, spelled out
    h = got.view(np.float16)
    assert h[0] == 1.0 and h[1] == np.float16(1 + 2.0 ** -9)                # ties to even, both ways
    assert h[2] == 65504 and h[3] == 65504 and np.isposinf(h[4]) and np.isneginf(h[5])
    assert got[11] == 0 and got[12] == 1 and got[13] == 0x8000             # 2^-25 -> 0, its successor -> 2^-24, sign kept
    assert got[14] == 0 and got[15] == 0x8000                              # +-0
    for m in (1, 4095, 4096, 4097):                                          # the wrapper, every tail length
        from m3d import headstore
        hh = headstore.to_half(d[:m].reshape(1, m))
        assert hh.dtype == torch.float16 and tuple(hh.shape) == (1, m)
        a, b = hh.cpu().numpy().view(np.uint16).ravel(), want[:m].view(np.uint16)
        assert np.array_equal(a[~nan[:m]], b[~nan[:m]])


# --------------------------------------------------------------------------- row counts
@pytest.mark.parametrize("row_bits", [27, 64, 21952])
def test_bits_row_counts(cuda, row_bits):
    lib, L = _L()
    rows = 5
    rng = np.random.default_rng(row_bits)
    flat = (rng.uniform(size=rows * row_bits) < 0.3).astype(np.uint8)
    flat[:row_bits] = 1                                                     # a full row, and ...
    flat[2 * row_bits:3 * row_bits] = 0                                     # ... an empty one between set neighbours
    flat[2 * row_bits - 1] = flat[3 * row_bits] = 1
    bits = np.packbits(flat)
    pad = 8 * bits.size - flat.size
    if pad:
        bits[-1] |= (1 << pad) - 1                                          # set padding bits must not be counted
    want = flat.reshape(rows, row_bits).sum(1).astype(np.int32)
    assert np.array_equal(want, np.unpackbits(np.packbits(flat))[:flat.size].reshape(rows, row_bits).sum(1))
    d = torch.from_numpy(bits).to(cuda)
    got = twice(lambda out: lib.check(L.m3d_bits_row_counts(d.data_ptr(), rows, row_bits, out, lib.stream()),
                                      "counts"), 4 * rows, np.int32, cuda)
    assert np.array_equal(got, want)
    from m3d import headstore
    assert np.array_equal(headstore.bits_row_counts(d, rows, row_bits).cpu().numpy(), want)
    # count / row_bits in float32 is numpy's float32 mean of the 0/1 row
    cov = got.astype(np.float32) / np.float32(row_bits)
    assert all(np.float32(c) == flat.reshape(rows, row_bits)[r].astype(np.float32).mean() for r, c in enumerate(cov))


# --------------------------------------------------------------------------- unpack-gather
def _gather_want(src, sel, M):
    from m3d.headstore import index_table
    i0, i1, i2 = (index_table(s, m) for s, m in zip(src.shape[1:4], M))
    out = src[np.maximum(sel, 0)][:, i0][:, :, i1][:, :, :, i2].astype(np.float32)
    out[np.asarray(sel) < 0] = 0
    return out


def _gather_call(fn, d_src, shape, sel, M, cuda):
    lib, L = _L()
    from m3d.headstore import index_table
    R, S0, S1, S2, C = shape
    tabs = [torch.from_numpy(index_table(s, m).astype(np.int32)).to(cuda) for s, m in zip((S0, S1, S2), M)]
    d_sel = torch.from_numpy(np.asarray(sel, np.int32)).to(cuda)
    n = len(sel) * M[0] * M[1] * M[2] * C
    got = twice(lambda out: lib.check(fn(d_src.data_ptr(), R, S0, S1, S2, C, d_sel.data_ptr(), len(sel),
                                         tabs[0].data_ptr(), tabs[1].data_ptr(), tabs[2].data_ptr(), *M, out,
                                         lib.stream()), "gather"), 4 * n, np.float32, cuda)
    return got.reshape(len(sel), *M, C)


SEL = [1, 4, -1, 1, 0]          # a repeat, a padding row, the last row
GATHER_CASES = [((5, 4, 3, 2, 1), (3, 3, 2)), ((5, 4, 3, 2, 1), (4, 3, 2)), ((5, 4, 3, 2, 8), (3, 3, 2)),
                ((5, 4, 3, 2, 8), (4, 3, 2)),
                ((5, 4, 3, 2, 3), (3, 4, 3)),            # C % 4 != 0 with C > 1: elements straddle bytes; upsampling
                ((5, 2, 2, 5, 256), (2, 2, 5)),          # a row of M2 * C / 4 = 320 vectors: two steps along the row, two rows
                ((5, 1, 1, 5, 256), (1, 1, 5)),          # ... with an odd number of rows: a dead step
                ((5, 2, 2, 4, 256), (2, 2, 4)),          # ... of exactly 256: one step along the row, four rows
                ((5, 2, 1, 17, 256), (2, 1, 17)),        # ... of more than 4 * 256: a second workgroup along the row
                ((5, 2, 1, 50, 3), (2, 1, 50)),          # one row per step without the vector path (150 elements, C = 3)
                ((5, 2, 1, 50, 12), (2, 1, 50)),         # ... with it, C / 4 = 3 no power of two
                ((5, 3, 2, 2, 256), (2, 2, 1)),          # exactly 64 vectors: four rows per workgroup and step
                ((5, 4, 3, 2, 1), (12, 12, 2))]          # 720 rows of 2: 128 rows per step, a second, partial workgroup


@pytest.mark.parametrize("shape,M", GATHER_CASES)
def test_unpack_gather_bits(cuda, shape, M):
    _, L = _L()
    rng = np.random.default_rng(sum(shape) + sum(M))
    src = (rng.uniform(size=shape) < 0.5).astype(np.uint8)
    d = torch.from_numpy(np.packbits(src)).to(cuda)
    got = _gather_call(L.m3d_unpack_gather_bits, d, shape, SEL, M, cuda)
    want = _gather_want(src, np.array(SEL), M)
    assert np.array_equal(got, want) and set(np.unique(got)) <= {0.0, 1.0}
    assert not got[2].any() and got[0].any()
    from m3d import headstore
    w = headstore.unpack_gather(d, shape, SEL, M)
    assert tuple(w.shape) == (len(SEL), *M, shape[4]) and np.array_equal(w.cpu().numpy(), want)
    with pytest.raises(ValueError, match="row 5 of 5"):
        headstore.unpack_gather(d, shape, [0, 5], M)


@pytest.mark.parametrize("shape,M", GATHER_CASES)
def test_unpack_gather_f16(cuda, shape, M):
    _, L = _L()
    rng = np.random.default_rng(sum(shape) + sum(M) + 1)
    with np.errstate(over="ignore"):
        src = (rng.normal(size=shape) * 10.0 ** rng.uniform(-7, 4, shape)).astype(np.float16)  # subnormals to inf
    src.reshape(-1)[:4] = [np.inf, -0.0, 6e-8, -65504]
    d = torch.from_numpy(src).to(cuda)
    got = _gather_call(L.m3d_unpack_gather_f16, d, shape, SEL, M, cuda)
    want = _gather_want(src, np.array(SEL), M)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))                           # widened exactly
    from m3d import headstore
    assert np.array_equal(headstore.unpack_gather(d, shape, SEL, M).cpu().numpy().view(np.uint32),
                          want.view(np.uint32))
    pad = headstore.unpack_gather(d, shape, [-1, -1])
    assert tuple(pad.shape) == (2, *shape[1:]) and not pad.any()


# --------------------------------------------------------------------------- end to end
SGD = {"name": "SGD", "parameters": {"learning_rate": 0.01, "momentum": 0.9}}
GT_BOXES = np.array([[4, 4, 0, 32, 36, 64], [30, 8, 0, 60, 34, 64], [12, 36, 0, 40, 62, 64]], np.int32)


def _config(**kw):
    """The configuration of test_train_heads_both_heads_on_a_toy_volume (tests/test_gpu_mask_head_train.py)."""
    from m3d.config import synthetic_mrcnn_config
    d = dict(PRE_NMS_LIMIT=2000, POST_NMS_ROIS_TRAINING=300, POST_NMS_ROIS_INFERENCE=64, TRAIN_ROIS_PER_IMAGE=12,
             ROI_POSITIVE_RATIO=0.5, USE_MINI_MASK=False, MASK_SHAPE=[28, 28, 28], DETECTION_MAX_INSTANCES=8,
             HEAD_CONV_CHANNEL=64, RPN_POSITIVE_IOU=0.02, RPN_NEGATIVE_IOU=0.01, MIN_POSITIVE_TARGETS=0,
             TARGET_RATIO=1.0)                       # every image of the split (the default keeps a fifth)
    d.update(kw)
    return synthetic_mrcnn_config(64, depth=64, **d)


def _gt(ds, image_id, cuda):
    """The arguments of _head_targets / train_heads for one image, as head_target_generation builds them."""
    from m3d.model import compose_image_meta
    image = ds.load_image(image_id, device=cuda)[None]
    boxes, class_ids, masks = ds.load_data(image_id)
    meta = compose_image_meta(image_id, (64, 64, 64, 1), (64, 64, 64, 1), (0, 0, 0, 64, 64, 64), 1.0,
                              np.ones(2, np.int32))
    return (image, torch.from_numpy(meta[None]).to(cuda), torch.from_numpy(class_ids.astype(np.int32)[None]).to(cuda),
            torch.from_numpy(boxes.astype(np.float32)[None]).to(cuda), torch.from_numpy((masks != 0)[None]).to(cuda))


@pytest.fixture(scope="module")
def world(cuda, tmp_path_factory):
    """A two-image dataset in ToyDataset's layout (the 64^3 synthetic volume as
    a uint16 stack, the three boxes and their box-filling masks), a model, and
    the stored head targets generated from it."""
    from m3d.dataset import ToyDataset, ToyHeadDataset
    from m3d.heads import MaskRCNN
    from m3d.model import synthetic_volume
    from m3d.tiff import imwrite
    root = str(tmp_path_factory.mktemp("head_world"))
    os.makedirs(os.path.join(root, "datasets"))
    rows = []
    for i in range(2):
        v = synthetic_volume(64, 64, seed=i)[0, ..., 0].numpy()                    # [H,W,D] in (-1, 1)
        raw = np.round((v.transpose(2, 0, 1) + 1.0) * 32767.0).astype(np.uint16)  # (Z,Y,X)
        paths = [os.path.join(root, f"vol_{i}{ext}") for ext in (".tiff", ".dat", ".pickle.bz2")]
        imwrite(paths[0], raw)
        masks = np.zeros((64, 64, 64, len(GT_BOXES)), bool)                        # (Z,Y,X,N)
        with open(paths[1], "w") as f:
            for g, (y1, x1, z1, y2, x2, z2) in enumerate(GT_BOXES):
                f.write(f"1 {z1} {y1} {x1} {z2} {y2} {x2}\n")
                masks[z1:z2, y1:y2, x1:x2, g] = True
        with bz2.BZ2File(paths[2], "wb") as f:
            pickle.dump(masks, f)
        rows.append(paths)
    with open(os.path.join(root, "datasets", "train.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["images", "cabs", "masks"])
        w.writerows(rows)
    ds = ToyDataset()
    ds.load_dataset(root, is_train=True)
    ds.prepare()
    cfg = _config()
    model = MaskRCNN(cfg, device=cuda, seed=2)
    out_dir = os.path.join(root, "head_targets")
    report = model.head_target_generation(ds, out_dir, "train", seed=5)
    hds = ToyHeadDataset(config=cfg)
    hds.load_dataset(out_dir, is_train=True)
    hds.prepare()
    return {"ds": ds, "cfg": cfg, "model": model, "out_dir": out_dir, "report": report, "hds": hds, "root": root}


def test_generation_then_generator_reproduces_the_direct_targets(cuda, world):
    from m3d import headstore
    from m3d.generator import HeadGenerator
    model, ds, report = world["model"], world["ds"], world["report"]
    assert report["processed"] == 2 and report["saved"] == 2 and report["skipped"] == []
    with open(report["csv"], newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == list(headstore.COLUMNS) and len(rows) == 3
    assert rows[1] == [os.path.join(world["out_dir"], c, "vol_0.npz") for c in headstore.COLUMNS]
    assert all(os.path.isfile(p) for r in rows[1:] for p in r)
    gen = HeadGenerator(world["cfg"], world["hds"], cuda, shuffle=False, training=False)
    assert len(gen) == 2
    positives = []
    for k in range(2):
        args = _gt(ds, k, cuda)
        with torch.no_grad():
            _, rois, _, ids, tbox, tmask, maps = model._head_targets(*args, 5 + k)
            pooled = model.roi_align_classifier([rois, args[1]] + maps)
            mpooled = model.roi_align_mask([rois, args[1]] + maps)
        item = gen[k]
        assert [tuple(t.shape) for t in item] == [(1, 12, 7, 7, 7, 256), (1, 12, 14, 14, 14, 256), (1, 18), (1, 12),
                                                  (1, 12, 6), (1, 12, 28, 28, 28)]
        assert all(t.is_cuda for t in item) and item[3].dtype == torch.int32
        want_ra = pooled.cpu().numpy().astype(np.float16).astype(np.float32)
        assert np.array_equal(item[0].cpu().numpy().view(np.uint32), want_ra.view(np.uint32))
        # (the untrained trunk's features stay below 0.5, so these are zeros here; the generator test
        # below and the kernel tests above compare mixed bits)
        assert torch.equal(item[1], (mpooled > 0.5).float())
        assert torch.equal(item[2], args[1])
        assert torch.equal(item[3], ids) and torch.equal(item[4], tbox)
        assert torch.equal(item[5], (tmask > 0.5).float())
        assert torch.equal(gen.last["rois"], rois) and gen.last["image_id"] == k
        assert list(gen.last["sel"]) == list(range(12))
        assert float(item[0].abs().max()) > 0
        positives.append((int((ids > 0).sum()), int(item[5].sum()), int(item[1].sum())))
        if positives[-1][0]:
            assert positives[-1][1] > 0                                    # a positive ROI carries a mask
        # the host reader sees the same arrays
        h = world["hds"].load_data(k)
        assert np.array_equal(h[1], want_ra[0]) and np.array_equal(h[5][..., 0], item[5][0].cpu().numpy())
    print("per image (positive ROIs, target-mask bits, mask_aligned bits):", positives)


def test_generation_skips_images_below_min_positive_targets(cuda, world, tmp_path):
    from m3d import headstore
    model = world["model"]
    model.config.MIN_POSITIVE_TARGETS = 10 ** 6
    try:
        report = model.head_target_generation(world["ds"], str(tmp_path), "test", seed=5)
    finally:
        model.config.MIN_POSITIVE_TARGETS = 0
    assert report["processed"] == 2 and report["saved"] == 0
    assert [n for n, _ in report["skipped"]] == ["vol_0", "vol_1"]
    with open(os.path.join(str(tmp_path), "datasets", "test.csv"), newline="") as f:
        assert list(csv.reader(f)) == [list(headstore.COLUMNS)]
    assert not os.path.exists(os.path.join(str(tmp_path), "rois"))


def test_train_heads_is_train_heads_on_features(cuda, world):
    """The refactoring guard: in deterministic mode, train_heads_on_features on
    the float32 features of _head_targets leaves the store, the moments and
    the head BN statistics bit-equal to train_heads."""
    from m3d import _lib
    from m3d.heads import MaskRCNN
    from m3d.optim import KerasOptimizer
    cfg, args = world["cfg"], _gt(world["ds"], 0, cuda)
    _lib.set_deterministic(True, scratch_bytes=64 << 20, device=cuda)
    try:
        a, b = MaskRCNN(cfg, device=cuda, seed=2), MaskRCNN(cfg, device=cuda, seed=2)
        ra = a.train_heads(*args, KerasOptimizer(SGD), seed=5)
        with torch.no_grad():
            _, rois, _, ids, tbox, tmask, maps = b._head_targets(*args, 5)
            pooled = b.roi_align_classifier([rois, args[1]] + maps)
            mpooled = b.roi_align_mask([rois, args[1]] + maps)
        rb = b.train_heads_on_features(pooled, mpooled, args[1], ids, tbox, tmask, KerasOptimizer(SGD))
    finally:
        _lib.set_deterministic(False)
    assert torch.equal(a.store.flat.detach(), b.store.flat.detach())
    assert torch.equal(a.store.moments, b.store.moments) and torch.equal(a.store.grad_flat, b.store.grad_flat)
    for x, y in zip(a.store.bns, b.store.bns):
        assert torch.equal(x.moving_mean, y.moving_mean) and torch.equal(x.moving_variance, y.moving_variance)
    assert set(ra) == set(rb) | {"rois"} and torch.equal(ra["rois"], rois)
    for k in rb:
        assert torch.equal(ra[k], rb[k]), k
    assert float(ra["mrcnn_mask_loss"]) >= 0 and bool(torch.isfinite(ra["loss"]))


def test_a_training_step_on_a_stored_item(cuda, world):
    """train_heads_on_features on a HeadGenerator item: finite losses, and only
    the two heads' chunks move."""
    from m3d.generator import HeadGenerator
    from m3d.heads import MaskRCNN
    from m3d.optim import KerasOptimizer
    from m3d.params import CHUNK
    cfg = world["cfg"]
    model = MaskRCNN(cfg, device=cuda, seed=2)
    gen = HeadGenerator(cfg, world["hds"], cuda, seed=3)
    item = gen[0]
    lo, hi = model.classifier.chunk_range()[0], model.mask_head.chunk_range()[1]
    flat0 = model.store.flat.detach().clone()
    bn0 = [(bn.moving_mean.clone(), bn.moving_variance.clone()) for bn in model.store.bns]
    optimizer = KerasOptimizer(SGD)
    out = model.train_heads_on_features(*item, optimizer)
    assert optimizer.iterations == 1 and "rois" not in out
    for k in ("loss", "mrcnn_class_loss", "mrcnn_bbox_loss", "mrcnn_mask_loss"):
        assert bool(torch.isfinite(out[k])), k
    assert tuple(out["d_pooled"].shape) == tuple(item[0].shape)
    assert tuple(out["d_mask_pooled"].shape) == tuple(item[1].shape)
    flat = model.store.flat.detach()
    assert torch.equal(flat[:lo * CHUNK], flat0[:lo * CHUNK]) and torch.equal(flat[hi * CHUNK:], flat0[hi * CHUNK:])
    assert not torch.equal(flat[lo * CHUNK:hi * CHUNK], flat0[lo * CHUNK:hi * CHUNK])
    head_bns = [model.classifier.bn1, model.classifier.bn2] + [bn for _, bn in model.mask_head.convs.values()]
    for bn, (mm, mv) in zip(model.store.bns, bn0):
        same = torch.equal(bn.moving_mean, mm) and torch.equal(bn.moving_variance, mv)
        assert same != any(bn is h for h in head_bns), bn.name


def test_generator_resizes_and_balances_like_the_host_restatement(cuda, tmp_path):
    """Stored extents that differ from the configured ones (mask_aligned 5 -> 4,
    target_mask 4 -> 6) and more stored ROIs than TRAIN_ROIS_PER_IMAGE: the
    item is the numpy restatement of the reference's __getitem__ on
    ToyHeadDataset.load_data -- _resize_spatial's indexing, the coverages of
    the resized masks, the balanced selection with the same seed, zero padding
    -- and save_head_targets' files are numpy's astype / packbits."""
    import types
    from m3d import headstore
    from m3d.dataset import ToyHeadDataset
    from m3d.generator import HeadGenerator, select_head_rois
    rng = np.random.default_rng(9)
    R, T = 20, 8
    tci = np.array([1, 0] * 7 + [0] * 6, np.int32)
    pos = np.where(tci > 0)[0]
    tmask = np.zeros((R, 4, 4, 4), np.float32)
    tmask[pos[::2]] = rng.uniform(size=(len(pos[::2]), 4, 4, 4)) < 0.5           # four strong positives ...
    tmask[pos[1::2], 3, 3, 3] = 1                                                # ... and three weak ones (one voxel)
    a = {"rois": rng.uniform(0, 1, (R, 6)).astype(np.float32),
         "ra": rng.normal(size=(R, 3, 3, 3, 8)).astype(np.float32),
         "ma": rng.uniform(0, 1, (R, 5, 5, 5, 8)).astype(np.float32),
         "tb": rng.normal(size=(R, 6)).astype(np.float32),
         "tm": tmask}
    dev = {k: torch.from_numpy(v).to(cuda) for k, v in a.items()}
    paths = headstore.save_head_targets(str(tmp_path), "vol", dev["rois"], dev["ra"], dev["ma"],
                                        torch.from_numpy(tci).to(cuda), dev["tb"], dev["tm"])
    with np.load(paths[1]) as z:
        assert np.array_equal(z["rois_aligned"].view(np.uint16), a["ra"].astype(np.float16).view(np.uint16))
    with np.load(paths[2]) as z:
        assert np.array_equal(z["mask_bits"], np.packbits(a["ma"] > 0.5)) and z["mask_shape"].tolist() == [R, 5, 5, 5, 8]
    with np.load(paths[5]) as z:
        assert np.array_equal(z["tm_bits"], np.packbits(a["tm"] > 0.5)) and z["tm_shape"].tolist() == [R, 4, 4, 4]
    headstore.append_csv_row(headstore.write_csv_header(str(tmp_path), "train"), paths)
    cfg = types.SimpleNamespace(TRAIN_ROIS_PER_IMAGE=T, MASK_POOL_SIZE=4, MASK_SHAPE=[6, 6, 6], NUM_CLASSES=2,
                                IMAGE_SHAPE=np.array([64, 64, 16, 1]), HEAD_SHUFFLE_ROIS=True, HEAD_BALANCE_POS=True,
                                HEAD_POS_FRAC=0.5, HEAD_MIN_POSITIVE_COVERAGE=0.06)
    ds = ToyHeadDataset(config=cfg)
    ds.load_dataset(str(tmp_path))
    ds.prepare()
    rois, ra, ma, ids, tb, tm = ds.load_data(0)

    def resize(x, M):
        i = [headstore.index_table(s, M) for s in x.shape[1:4]]
        return x[:, i[0]][:, :, i[1]][:, :, :, i[2]]

    ma_r, tm_r = resize(ma, 4), resize(tm, 6)
    cov = np.array([tm_r[i].mean() for i in range(R)], np.float32)
    assert (cov[tci > 0] < 0.06).any() and (cov[tci > 0] >= 0.06).any()
    for seed in (0, 1):
        gen = HeadGenerator(cfg, ds, cuda, seed=seed, shuffle=False, training=True)
        item = gen[0]
        sel = select_head_rois(ids, cov, T, cfg, np.random.RandomState(seed), True)
        assert np.array_equal(gen.last["sel"], sel) and sel.min() >= 0
        assert int((ids[sel] > 0).sum()) == 4 and (cov[sel][ids[sel] > 0] >= 0.06).all()
        for got, want in zip(item, (ra[sel], ma_r[sel], None, ids[sel], tb[sel], tm_r[sel][..., 0])):
            if want is not None:
                assert tuple(got.shape) == (1,) + want.shape and np.array_equal(got[0].cpu().numpy(), want)
        assert np.array_equal(gen.last["rois"][0].cpu().numpy(), rois[sel])
    # fewer stored ROIs than T: the tail is zero rows
    few = types.SimpleNamespace(**{**vars(cfg), "TRAIN_ROIS_PER_IMAGE": R + 3})
    gen = HeadGenerator(few, ds, cuda, seed=0, shuffle=False, training=False)
    item = gen[0]
    assert list(gen.last["sel"]) == list(range(R)) + [-1] * 3
    assert np.array_equal(item[1][0, :R].cpu().numpy(), ma_r) and np.array_equal(item[0][0, :R].cpu().numpy(), ra)
    assert all(not t[0, R:].any() for i, t in enumerate(item) if i != 2)
    assert np.array_equal(item[3][0, :R].cpu().numpy(), ids) and item[3].dtype == torch.int32
