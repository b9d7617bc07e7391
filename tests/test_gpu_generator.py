"""m3d.generator.RPNGenerator on a small dataset written in the reference's
on-disk layout: three 64 x 64 x 16 uint16 volumes, the third without boxes.
The image bar is the one of tests/test_gpu_preprocess.py (no larger than the
float32 evaluation's error against the float64 restatement tests/normref.py);
targets, flips and sequences are compared bit for bit."""
import bz2
import csv
import os
import pickle

import numpy as np
import pytest
import torch

import normref as N

pytestmark = pytest.mark.gpu

S, D = 64, 16
BOXES = [np.array([[4, 4, 2, 32, 36, 10], [30, 8, 5, 60, 34, 15], [12, 36, 0, 40, 62, 8]], np.float32),
         np.array([[8, 10, 1, 40, 30, 9], [34, 30, 6, 62, 60, 16]], np.float32),
         np.zeros((0, 6), np.float32)]


def _cfg(**kw):
    from m3d.config import synthetic_rpn_config
    d = dict(RPN_POSITIVE_IOU=0.3, RPN_NEGATIVE_IOU=0.1, RPN_TRAIN_ANCHORS_PER_IMAGE=256, PRE_NMS_LIMIT=2000,
             POST_NMS_ROIS_TRAINING=300, AUGMENT=False, RPN_AUGMENT_GT=False, AUG_BRIGHTNESS_DELTA=0.0)
    d.update(kw)
    return synthetic_rpn_config(S, depth=D, **d)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """(dataset, raw stacks): <root>/datasets/train.csv, (Z,Y,X) TIFFs, .dat
    rows `class z1 y1 x1 z2 y2 x2`, bz2-pickled (Z,Y,X,N) masks."""
    from m3d.dataset import ToyDataset
    from m3d.tiff import imwrite
    root = str(tmp_path_factory.mktemp("rpn_generator"))
    os.makedirs(os.path.join(root, "datasets"))
    raws, rows = [], []
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
        raws.append(raw)
        rows.append(paths)
    with open(os.path.join(root, "datasets", "train.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["images", "cabs", "masks"])
        w.writerows(rows)
    ds = ToyDataset()
    ds.load_dataset(root, is_train=True)
    ds.prepare()
    return ds, raws


def _anchors(cfg, cuda):
    from m3d.anchors import get_anchors
    return torch.from_numpy(get_anchors(cfg)).to(cuda)


def _builder_targets(cfg, cuda, boxes_px, seed):
    """A fresh RPNTargetBuilder on pixel boxes normalised as the generator does."""
    from m3d.targets import RPNTargetBuilder
    gt = np.clip(boxes_px / np.array([S, S, D, S, S, D], np.float32), 0.0, 1.0).astype(np.float32)
    t = RPNTargetBuilder(_anchors(cfg, cuda), cfg, max_gt=16)(torch.from_numpy(gt).to(cuda), seed=seed)
    return t.match.clone(), t.bbox.clone()


def _gen(cfg, data, cuda, anchors=None, **kw):
    from m3d.generator import RPNGenerator
    return RPNGenerator(cfg, data[0], _anchors(cfg, cuda) if anchors is None else anchors, cuda, **kw)


def test_plain_item_is_the_normalised_image_and_the_builder_targets(cuda, data):
    from m3d.dataset import normalize_image
    from m3d.model import DeviceRPNTargets
    cfg = _cfg()
    gen = _gen(cfg, data, cuda, shuffle=False)
    assert len(gen) == 3
    for i in (0, 1):
        image, t = gen[i]
        assert isinstance(t, DeviceRPNTargets) and tuple(image.shape) == (1, S, S, D, 1) and image.is_cuda
        got = image[0, ..., 0].cpu().numpy()
        ref, _ = N.normalize(data[1][i])
        bar = float(np.abs(N.normalize_f32(data[1][i]).astype(np.float64) - ref).max())
        err = float(np.abs(got.astype(np.float64) - ref).max())
        print("image", i, "gpu max error", err, "float32 evaluation", bar, "bit-equal to the host path",
              float((got == normalize_image(data[1][i])[..., 0]).mean()))
        assert err <= bar
        assert gen.last["image_id"] == i and gen.last["tries"] == 0 and np.array_equal(gen.last["boxes"], BOXES[i])
        match, bbox = _builder_targets(cfg, cuda, BOXES[i], gen.last["target_seed"])
        assert torch.equal(t.match, match) and torch.equal(t.bbox, bbox)
        assert int((t.match == 1).sum()) > 0


def test_flips_move_image_and_boxes_together(cuda, data):
    plain = _gen(_cfg(), data, cuda, shuffle=False)
    cfg = _cfg(AUGMENT=True, AUG_PROB=1.0, AUG_FLIP_Y=True, AUG_FLIP_X=True, AUG_FLIP_Z=True,
               AUG_BRIGHTNESS_DELTA=0.0, AUG_GAUSS_NOISE_STD=0.0)
    gen = _gen(cfg, data, cuda, shuffle=False)
    for i in (0, 1):
        want = plain[i][0].cpu().numpy()
        image, t = gen[i]
        assert np.array_equal(image.cpu().numpy(), want[:, ::-1, ::-1, ::-1])
        flipped = N.flip_boxes(BOXES[i], (S, S, D), 7)
        assert np.array_equal(gen.last["boxes"], flipped)
        match, bbox = _builder_targets(cfg, cuda, flipped, gen.last["target_seed"])
        assert torch.equal(t.match, match) and torch.equal(t.bbox, bbox)
    # MODE other than "training": no augmentation, as load_image_gt
    off = _gen(_cfg(AUGMENT=True, AUG_PROB=1.0, MODE="targeting"), data, cuda, shuffle=False)
    assert np.array_equal(off[0][0].cpu().numpy(), plain[0][0].cpu().numpy())


def _epochs(gen, n=2):
    seq = []
    for _ in range(n):
        for i in range(len(gen)):
            image, t = gen[i]
            seq.append((gen.last["image_id"], gen.last["boxes_for_rpn"].copy(), image.clone(), t.match.clone(),
                        t.bbox.clone()))
        gen.on_epoch_end()
    return seq


def test_same_seed_same_sequence(cuda, data):
    cfg = _cfg(AUGMENT=True, AUG_PROB=0.5, AUG_FLIP_Z=True, AUG_BRIGHTNESS_DELTA=0.03, AUG_GAUSS_NOISE_STD=0.01,
               RPN_AUGMENT_GT=True, RPN_GT_JITTER_PER_BOX=3, RPN_GT_JITTER_SCALE_SIGMA=0.1,
               RPN_GT_JITTER_TRANS=[2, 2, 1], RPN_GT_JITTER_IOU_THR=0.4)
    a, b = (_epochs(_gen(cfg, data, cuda, seed=5)) for _ in range(2))
    c = _epochs(_gen(cfg, data, cuda, seed=6))
    assert len(a) == 6
    for x, y in zip(a, b):
        assert x[0] == y[0] and np.array_equal(x[1], y[1])
        assert all(torch.equal(u, v) for u, v in zip(x[2:], y[2:]))
    assert any(len(x[1]) > len(BOXES[x[0]]) for x in a), "no jittered box was kept in six items"
    assert any(x[0] != y[0] or not torch.equal(x[2], y[2]) for x, y in zip(a, c))
    # the shuffle: both epochs visit a permutation of the ids (the empty image is replaced)
    from m3d.generator import RPNGenerator
    g = RPNGenerator(cfg, data[0], _anchors(cfg, cuda), cuda, seed=5)
    first = g.image_ids.copy()
    g.on_epoch_end()
    assert sorted(first) == sorted(g.image_ids) == [0, 1, 2]
    ref = np.random.RandomState(5)
    ids = np.arange(3)
    ref.shuffle(ids)
    assert np.array_equal(first, ids)


def test_image_without_boxes_is_replaced(cuda, data):
    gen = _gen(_cfg(), data, cuda, shuffle=False, seed=1)
    image, t = gen[2]
    assert gen.last["image_id"] in (0, 1) and 1 <= gen.last["tries"] <= 5 and len(gen.last["boxes"]) > 0
    want = _gen(_cfg(), data, cuda, shuffle=False)[gen.last["image_id"]][0]
    assert torch.equal(image, want) and int((t.match == 1).sum()) > 0


def test_train_step_on_a_generator_item(cuda, data):
    from m3d.model import RPN
    cfg = _cfg(AUGMENT=True, AUG_PROB=0.5, AUG_BRIGHTNESS_DELTA=0.03, RPN_AUGMENT_GT=True)
    model = RPN(cfg, device=cuda, seed=1)
    gen = _gen(cfg, data, cuda, anchors=model.anchors.reshape(-1, 6), seed=3)
    image, targets = gen[0]
    r = model.train_step(image, targets)
    torch.cuda.synchronize()
    assert torch.isfinite(r["loss"]).item() and float(r["loss"]) > 0
